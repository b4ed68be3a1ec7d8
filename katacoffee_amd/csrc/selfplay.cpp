// Host side of the self-play engine: device allocation, the round loop and the
// row drain.  Replaces the reference's per-thread game loop (selfplay.cpp:262-330
// gameLoop, Play::runGame play.cpp:1146-1701) and NNEvaluator batching
// (nneval.cpp:386-567): all games advance together, one playout per round.
#include "selfplay.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace kc {

static int nextPow2(int v) {
  int p = 1;
  while(p < v)
    p <<= 1;
  return p;
}

SP toSP(const coffee_search_params& p) {
  SP s;
  s.maxVisits = p.max_visits;
  s.cpuct = p.cpuct_exploration;
  s.cpuctLog = p.cpuct_exploration_log;
  s.cpuctBase = p.cpuct_exploration_base;
  s.fpuRedMax = p.fpu_reduction_max;
  s.rootFpuRedMax = p.root_fpu_reduction_max;
  s.fpuLossProp = p.fpu_loss_prop;
  s.rootFpuLossProp = p.root_fpu_loss_prop;
  s.fpuByVisited = p.fpu_parent_weight_by_visited_policy;
  s.fpuByVisitedPow = p.fpu_parent_weight_by_visited_policy_pow;
  s.valueWeightExp = p.value_weight_exponent;
  s.rootNoise = p.root_noise_enabled;
  s.dirConc = p.root_dirichlet_noise_total_concentration;
  s.dirWeight = p.root_dirichlet_noise_weight;
  s.rootTemp = p.root_policy_temperature;
  s.rootTempEarly = p.root_policy_temperature_early;
  s.rootDesiredCoeff = p.root_desired_per_child_visits_coeff;
  s.rootSyms = p.root_num_symmetries_to_sample;
  s.moveTemp = p.chosen_move_temperature;
  s.moveTempEarly = p.chosen_move_temperature_early;
  s.moveTempHalflife = p.chosen_move_temperature_halflife;
  s.moveSubtract = p.chosen_move_subtract;
  s.movePrune = p.chosen_move_prune;
  s.useLcb = p.use_lcb_for_selection;
  s.lcbStdevs = p.lcb_stdevs;
  s.minVisitPropLcb = p.min_visit_prop_for_lcb;
  s.svbFactor = p.subtree_value_bias_factor;
  s.svbExp = p.subtree_value_bias_weight_exponent;
  s.svbFreeProp = p.subtree_value_bias_free_prop;
  s.useGraph = p.use_graph_search;
  s.cheapProb = p.cheap_search_prob;
  s.cheapVisits = p.cheap_search_visits;
  s.cheapWeight = p.cheap_search_target_weight;
  s.reduceVisits = p.reduce_visits;
  s.reduceThreshold = p.reduce_visits_threshold;
  s.reduceLookback = p.reduce_visits_threshold_lookback;
  s.reducedMin = p.reduced_visits_min;
  s.reducedWeight = p.reduced_visits_weight;
  s.policySurpriseWeight = p.policy_surprise_data_weight;
  s.valueSurpriseWeight = p.value_surprise_data_weight;
  s.initPolicy = p.init_games_with_policy;
  s.initAreaProp = p.policy_init_area_prop;
  s.initTemp = p.policy_init_area_temperature;
  s.earlyForkProb = p.early_fork_game_prob;
  s.earlyForkMoveProp = p.early_fork_game_expected_move_prop;
  s.forkProb = p.fork_game_prob;
  s.forkMinChoices = p.fork_game_min_choices;
  s.earlyForkMaxChoices = p.early_fork_game_max_choices;
  s.forkMaxChoices = p.fork_game_max_choices;
  s.sideProb = p.side_position_prob;
  s.recordTree = p.record_tree_positions;
  s.recordTreeThreshold = p.record_tree_threshold;
  s.recordTreeWeight = p.record_tree_target_weight;
  return s;
}

// Bytes of one staged row (kStageRows; rows.py FIELDS): bin, glob, pol, gtgt, value, meta.
int rowBytes(int A) {
  const int pb = (A + 7) / 8;
  return NUM_SPATIAL * pb + 4 + 2 * 4 * A * 2 + 64 * 4 + 5 * A + 16;
}

// Dynamic LDS of the commit kernel (kCommit's policy scratch, live-node bits and BFS queue).
size_t commitLdsBytes(int cap) {
  size_t b = (size_t)MAX_P * 4 * 4 + 16;
  b += (size_t)(cap / 32) * 4 + (size_t)cap * 2;
  return (b + 15) / 16 * 16;
}

template <class T>
static T* devAlloc(std::vector<void*>& owned, size_t count, bool zero = true) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  KC_HIP(hipMalloc(&p, bytes));
  owned.push_back(p);
  if(zero)
    KC_HIP(hipMemset(p, 0, bytes));
  return reinterpret_cast<T*>(p);
}

// The settings match play rejects (DESIGN.md "Match play"): each side searches with its own
// net from a cleared tree, and no training rows are made.
Unc toUnc(const coffee_uncertainty_params& p) {
  // setup.cpp:539-562 ranges; !(a <= x && x <= b) also rejects NaN
  auto in = [](float x, float lo, float hi) { return x >= lo && x <= hi; };
  if(p.use_uncertainty != 0 && p.use_uncertainty != 1)
    throw std::invalid_argument("use_uncertainty must be 0 or 1");
  if(!in(p.uncertainty_coeff, 1e-4f, 1.0f))
    throw std::invalid_argument("uncertainty_coeff must be in [1e-4, 1]");
  if(!in(p.uncertainty_exponent, 0.0f, 2.0f))
    throw std::invalid_argument("uncertainty_exponent must be in [0, 2]");
  if(!in(p.uncertainty_max_weight, 1.0f, 100.0f))
    throw std::invalid_argument("uncertainty_max_weight must be in [1, 100]");
  return Unc{p.use_uncertainty, p.uncertainty_coeff, p.uncertainty_exponent, p.uncertainty_max_weight};
}

Expl toExpl(const coffee_exploration_params& p) {
  // !(a <= x && x <= b) also rejects NaN; the upper bounds reject +inf
  auto in = [](float x, float lo, float hi) { return x >= lo && x <= hi; };
  if(p.use_noise_pruning != 0 && p.use_noise_pruning != 1)
    throw std::invalid_argument("use_noise_pruning must be 0 or 1");
  if(!in(p.noise_prune_utility_scale, 0.001f, 10.0f))
    throw std::invalid_argument("noise_prune_utility_scale must be in [0.001, 10]");
  if(!in(p.noise_pruning_cap, 0.0f, FLT_MAX))
    throw std::invalid_argument("noise_pruning_cap must be finite and >= 0");
  if(!in(p.cpuct_utility_stdev_prior, 0.0f, 10.0f))
    throw std::invalid_argument("cpuct_utility_stdev_prior must be in [0, 10]");
  if(!in(p.cpuct_utility_stdev_prior_weight, 0.0f, 100.0f))
    throw std::invalid_argument("cpuct_utility_stdev_prior_weight must be in [0, 100]");
  if(!in(p.cpuct_utility_stdev_scale, 0.0f, 1.0f))
    throw std::invalid_argument("cpuct_utility_stdev_scale must be in [0, 1]");
  if(p.cpuct_utility_stdev_prior == 0.0f && p.cpuct_utility_stdev_scale > 0.0f)
    throw std::invalid_argument("cpuct_utility_stdev_prior must be > 0 with cpuct_utility_stdev_scale > 0");
  return Expl{p.use_noise_pruning,          p.noise_prune_utility_scale,        p.noise_pruning_cap,
              p.cpuct_utility_stdev_prior, p.cpuct_utility_stdev_prior_weight, p.cpuct_utility_stdev_scale};
}

RootSearch toRootSearch(const coffee_root_search_params& p) {
  // (the comparisons also reject NaN and +inf)
  if(!(p.wide_root_noise >= 0.0f && p.wide_root_noise <= 5.0f))
    throw std::invalid_argument("wide_root_noise must be in [0, 5]");
  if(!(p.futile_visits_threshold == 0.0f || (p.futile_visits_threshold >= 0.01f && p.futile_visits_threshold <= 1.0f)))
    throw std::invalid_argument("futile_visits_threshold must be 0 or in [0.01, 1]");
  return RootSearch{p.wide_root_noise, p.futile_visits_threshold};
}

void validateMatchConfig(const coffee_match_config& c) {
  if(c.x < 2 || c.y < 2 || c.x > MAX_LEN || c.y > MAX_LEN)
    throw std::invalid_argument("board size must be 2..10 x 2..10");
  if(c.win_len < 2 || c.win_len > std::max(c.x, c.y))
    throw std::invalid_argument("win_len must be in 2..max(x, y)");
  const coffee_search_params& sp = c.search;
  auto reject = [](bool bad, const char* name, const char* why) {
    if(bad)
      throw std::invalid_argument(std::string("match play: ") + name + " " + why);
  };
  const char* keeps = "must be off (a kept tree would hold the other net's evaluations)";
  const char* rows = "must be off (it exists only to make training rows)";
  reject(sp.cheap_search_prob > 0.0f, "cheap_search_prob", keeps);
  reject(sp.reduce_visits != 0, "reduce_visits", rows);
  reject(sp.early_fork_game_prob > 0.0f, "early_fork_game_prob", rows);
  reject(sp.fork_game_prob > 0.0f, "fork_game_prob", rows);
  reject(sp.side_position_prob > 0.0f, "side_position_prob", rows);
  reject(sp.record_tree_positions != 0, "record_tree_positions", rows);
  reject(sp.policy_surprise_data_weight != 0.0f, "policy_surprise_data_weight", rows);
  reject(sp.value_surprise_data_weight != 0.0f, "value_surprise_data_weight", rows);
}

int nodeCapFor(int nodeCap, int maxVisits) {
  const int cap = nodeCap > 0 ? nodeCap : std::max(2048, 3 * maxVisits);
  return (cap + 63) / 64 * 64;
}

void validateMatchOptions(const coffee_match_config& c, const coffee_match_options* o) {
  if(!o)
    return;
  if((o->per_side != 0 && o->per_side != 1) || (o->share_net != 0 && o->share_net != 1))
    throw std::invalid_argument("match options: per_side and share_net must be 0 or 1");
  if(o->share_net) {
    const char *a = c.model_path[0], *b = c.model_path[1];
    if((a == nullptr) != (b == nullptr) || (a && strcmp(a, b) != 0))
      throw std::invalid_argument("match options: share_net needs equal model_path[0] and model_path[1]");
  }
  if(!o->per_side)
    return;
  int maxVisits = 0;
  for(int i = 0; i < 2; i++) {
    const std::string side = "match options: side " + std::to_string(i) + ": ";
    const coffee_search_params& sp = o->side[i].search;
    try {
      coffee_match_config t = c;
      t.search = sp;
      validateMatchConfig(t);
      if(sp.max_visits < 1)
        throw std::invalid_argument("max_visits must be >= 1");
      if(sp.root_num_symmetries_to_sample < 1 || sp.root_num_symmetries_to_sample > 4)
        throw std::invalid_argument("root_num_symmetries_to_sample must be in 1..4");
      try {
        toUnc(o->side[i].unc);
      } catch(const std::invalid_argument& e) {
        throw std::invalid_argument(std::string("unc: ") + e.what());
      }
      // game-level settings are one per engine (bit patterns: a NaN equals itself here)
      if(sp.init_games_with_policy != c.search.init_games_with_policy)
        throw std::invalid_argument("init_games_with_policy must equal the config's search (a game-level setting)");
      if(memcmp(&sp.policy_init_area_prop, &c.search.policy_init_area_prop, sizeof(float)) != 0)
        throw std::invalid_argument("policy_init_area_prop must equal the config's search (a game-level setting)");
      if(memcmp(&sp.policy_init_area_temperature, &c.search.policy_init_area_temperature, sizeof(float)) != 0)
        throw std::invalid_argument(
            "policy_init_area_temperature must equal the config's search (a game-level setting)");
    } catch(const std::invalid_argument& e) {
      throw std::invalid_argument(side + e.what());
    }
    maxVisits = std::max(maxVisits, sp.max_visits);
  }
  // the engine's rule for cfg->search.max_visits, on each side (the default pool comes from the larger)
  const int cap = nodeCapFor(c.node_cap, maxVisits);
  for(int i = 0; i < 2; i++)
    if(cap < o->side[i].search.max_visits + 4)
      throw std::invalid_argument("match options: side " + std::to_string(i) +
                                  ": max_visits: node_cap must exceed max_visits + 3");
}

// The self-play config a match engine is built on: one row of row buffer (never written).
coffee_selfplay_config SelfplayEngine::matchBase(const coffee_match_config& c, const coffee_match_options* o) {
  validateMatchConfig(c);  // before the first HIP call
  validateMatchOptions(c, o);
  coffee_selfplay_config b;
  memset(&b, 0, sizeof(b));
  b.x = c.x;
  b.y = c.y;
  b.win_len = c.win_len;
  b.num_games = c.num_games;
  b.node_cap = c.node_cap;
  b.row_capacity = 1;
  b.seed = c.seed;
  b.slot_base = c.slot_base;
  b.use_fake_net = 1;  // the two nets come from matchPaths
  b.commit_interval = c.commit_interval;
  b.search = c.search;
  b.nn_cache_log2 = c.nn_cache_log2;
  b.nn_batch_cap = c.nn_batch_cap;
  b.nn_precision = c.nn_precision;
  b.start_stagger = c.start_stagger;
  b.engines_per_device = c.engines_per_device;
  return b;
}

SelfplayEngine::SelfplayEngine(const coffee_match_config& c, const coffee_match_options* opts)
    : SelfplayEngine(matchBase(c, opts), c.model_path, opts) {}

// The settings analysis rejects: a query is one search from a cleared tree, and nothing is
// played or recorded, so every setting that keeps a tree, makes rows or plays opening moves
// has no meaning there.
void validateAnalysisConfig(const coffee_analysis_config& c) {
  if(c.x < 2 || c.y < 2 || c.x > MAX_LEN || c.y > MAX_LEN)
    throw std::invalid_argument("board size must be 2..10 x 2..10");
  if(c.win_len < 2 || c.win_len > std::max(c.x, c.y))
    throw std::invalid_argument("win_len must be in 2..max(x, y)");
  const coffee_search_params& sp = c.search;
  auto reject = [](bool bad, const char* name, const char* why) {
    if(bad)
      throw std::invalid_argument(std::string("analysis: ") + name + " " + why);
  };
  const char* keeps = "must be off (every query is searched from a cleared tree)";
  const char* rows = "must be off (it exists only to make training rows)";
  reject(sp.cheap_search_prob > 0.0f, "cheap_search_prob", keeps);
  reject(sp.reduce_visits != 0, "reduce_visits", rows);
  reject(sp.early_fork_game_prob > 0.0f, "early_fork_game_prob", rows);
  reject(sp.fork_game_prob > 0.0f, "fork_game_prob", rows);
  reject(sp.side_position_prob > 0.0f, "side_position_prob", rows);
  reject(sp.record_tree_positions != 0, "record_tree_positions", rows);
  reject(sp.policy_surprise_data_weight != 0.0f, "policy_surprise_data_weight", rows);
  reject(sp.value_surprise_data_weight != 0.0f, "value_surprise_data_weight", rows);
  reject(sp.init_games_with_policy != 0, "init_games_with_policy", "must be off (a query gives the position)");
  if(c.num_slots < 1)
    throw std::invalid_argument("analysis: num_slots must be >= 1");
  if(c.query_capacity < 1)
    throw std::invalid_argument("analysis: query_capacity must be >= 1");
  if(c.max_pv_len < 0 || c.max_pv_len > COFFEE_ANALYSIS_MAX_PV)
    throw std::invalid_argument("analysis: max_pv_len must be in 0.." + std::to_string(COFFEE_ANALYSIS_MAX_PV));
}

// the record layouts the Python mirror declares (katacoffee_amd ANALYSIS_*)
static_assert(sizeof(coffee_analysis_query) == 232 && sizeof(coffee_analysis_result) == 56 &&
                  sizeof(coffee_analysis_move) == 80,
              "analysis record layout");
static_assert(COFFEE_ANALYSIS_MAX_MOVES == MAX_AREA, "a query holds a full board of moves");

void validateAnalysisQuery(int x, int y, const coffee_analysis_query& q) {
  const int A = x * y, P = 4 * A;
  if(q.num_moves < 0 || q.num_moves > A || q.num_moves > COFFEE_ANALYSIS_MAX_MOVES)
    throw std::invalid_argument("analysis query " + std::to_string(q.id) + ": num_moves must be in 0.." +
                                std::to_string(A));
  for(int t = 0; t < q.num_moves; t++)
    if(q.moves[t] >= P)
      throw std::invalid_argument("analysis query " + std::to_string(q.id) + ": moves[" + std::to_string(t) +
                                  "] must be < " + std::to_string(P));
  if(q.max_visits < 0)
    throw std::invalid_argument("analysis query " + std::to_string(q.id) + ": max_visits must be >= 0");
}

coffee_selfplay_config SelfplayEngine::analysisBase(const coffee_analysis_config& c) {
  validateAnalysisConfig(c);  // before the first HIP call
  coffee_selfplay_config b;
  memset(&b, 0, sizeof(b));
  b.x = c.x;
  b.y = c.y;
  b.win_len = c.win_len;
  b.num_games = c.num_slots;
  b.node_cap = c.node_cap;
  b.row_capacity = 1;  // never written
  b.seed = c.seed;
  b.use_fake_net = c.model_path ? 0 : 1;
  b.model_path = c.model_path;
  b.commit_interval = c.commit_interval;
  b.search = c.search;
  b.nn_cache_log2 = c.nn_cache_log2;
  b.nn_batch_cap = c.nn_batch_cap;
  b.nn_precision = c.nn_precision;
  b.engines_per_device = c.engines_per_device;
  return b;
}

SelfplayEngine::SelfplayEngine(const coffee_analysis_config& c) : SelfplayEngine(analysisBase(c), nullptr) {
  SearchDev& d = hd_;
  d.analysisMode = 1;
  d.aCap = c.query_capacity;
  d.aMaxPv = c.max_pv_len;
  d.aQuery = devAlloc<coffee_analysis_query>(owned_, (size_t)d.aCap);
  d.aRes = devAlloc<coffee_analysis_result>(owned_, (size_t)d.aCap);
  d.aMoves = devAlloc<coffee_analysis_move>(owned_, (size_t)d.aCap * d.P);
  d.aCtr = devAlloc<unsigned long long>(owned_, AC_N);
  d.aSlot = devAlloc<AnalysisSlot>(owned_, (size_t)d.G);
  // root restrictions (rootmask.h): a zeroed ring entry is "no restriction"
  d.rootMask = devAlloc<uint32_t>(owned_, (size_t)d.G * ((d.P + 31) / 32));
  d.aRestrict = devAlloc<coffee_analysis_restrict>(owned_, (size_t)d.aCap);
  d.aRootInfo = devAlloc<coffee_analysis_root_info>(owned_, (size_t)d.aCap);
  KC_HIP(hipMemcpy(dd_, &d, sizeof(SearchDev), hipMemcpyHostToDevice));
  launchSelfplayInit(d, dd_, stream_);  // again, now in analysis mode: every slot idle
  KC_HIP(hipStreamSynchronize(stream_));
}

SelfplayEngine::SelfplayEngine(const coffee_selfplay_config& c, const char* const* matchPaths,
                               const coffee_match_options* matchOpts) {
  const bool perSide = matchPaths && matchOpts && matchOpts->per_side;
  const bool sharedNet = matchPaths && matchOpts && matchOpts->share_net;
  if(c.num_games <= 0)
    throw std::invalid_argument("num_games must be positive");
  if(c.num_games > 65535)  // kCompact packs two per-device game counts into 16-bit halves
    throw std::invalid_argument("num_games must be <= 65535 per device");
  const coffee_search_params& sp = c.search;
  if(sp.max_visits < 1 || sp.root_num_symmetries_to_sample < 1 || sp.root_num_symmetries_to_sample > 4)
    throw std::invalid_argument("search params: max_visits >= 1 and 1 <= root_num_symmetries_to_sample <= 4");
  // the reference's own checks (play.cpp:906-910, :925-930)
  if(sp.cheap_search_prob > 0.0f && (sp.cheap_search_visits <= 0 || sp.cheap_search_visits > sp.max_visits))
    throw std::invalid_argument("cheap_search_visits must be in [1, max_visits]");
  if(sp.reduce_visits && (sp.reduced_visits_min <= 0 || sp.reduced_visits_min > sp.max_visits))
    throw std::invalid_argument("reduced_visits_min must be in [1, max_visits]");
  if(sp.reduce_visits && (sp.reduce_visits_threshold < 0.0f || sp.reduce_visits_threshold >= 1.0f ||
                          sp.reduce_visits_threshold_lookback < 1 || sp.reduce_visits_threshold_lookback > 100))
    throw std::invalid_argument("reduce_visits_threshold must be in [0, 1) and lookback in [1, 100]");
  // playsettings.cpp:80-99 ranges
  auto unit = [](float x) { return x >= 0.0f && x <= 1.0f; };
  if(!unit(sp.cheap_search_prob) || !unit(sp.cheap_search_target_weight) || !unit(sp.reduced_visits_weight) ||
     !unit(sp.policy_surprise_data_weight) || !unit(sp.value_surprise_data_weight) ||
     sp.policy_surprise_data_weight + sp.value_surprise_data_weight > 1.0f)
    throw std::invalid_argument("play settings: probabilities and weights in [0, 1], surprise weights sum <= 1");
  if(sp.init_games_with_policy && (!unit(sp.policy_init_area_prop) || sp.policy_init_area_temperature < 0.1f ||
                                   sp.policy_init_area_temperature > 5.0f))
    throw std::invalid_argument("policy_init_area_prop in [0, 1], policy_init_area_temperature in [0.1, 5]");
  // playsettings.cpp:74-79 ranges; play.cpp:1783-1788 checks
  if(sp.early_fork_game_prob < 0.0f || sp.early_fork_game_prob > 0.5f || sp.fork_game_prob < 0.0f ||
     sp.fork_game_prob > 0.5f || !unit(sp.early_fork_game_expected_move_prop) || sp.fork_game_min_choices < 1 ||
     sp.early_fork_game_max_choices < sp.fork_game_min_choices || sp.fork_game_max_choices < sp.fork_game_min_choices ||
     sp.early_fork_game_max_choices > MAX_FORK_CHOICES || sp.fork_game_max_choices > MAX_FORK_CHOICES)
    throw std::invalid_argument("fork settings: probabilities in [0, 0.5], min <= max choices <= 100");
  if(!unit(sp.side_position_prob))
    throw std::invalid_argument("side_position_prob must be in [0, 1]");
  // play.cpp:1349-1350
  if(sp.record_tree_positions && sp.record_tree_target_weight > 1.0f)
    throw std::invalid_argument("record_tree_target_weight > 1");
  const DTables& ht = hostTables(c.x, c.y, c.win_len);
  T_ = deviceTables(c.x, c.y, c.win_len);
  commitInterval_ = c.commit_interval > 0 ? c.commit_interval : 8;
  // (per-side match settings: the default pool serves the larger side; validateMatchOptions
  // checked each side's max_visits against it)
  const int cap = nodeCapFor(c.node_cap, perSide ? std::max(matchOpts->side[0].search.max_visits,
                                                            matchOpts->side[1].search.max_visits)
                                                 : sp.max_visits);
  if(cap > 65535)
    throw std::invalid_argument("node_cap must be <= 65535");
  if(!perSide && cap < sp.max_visits + 4)  // (per side: validateMatchOptions)
    throw std::invalid_argument("node_cap must exceed max_visits + 3");
  const int G = c.num_games, P = ht.P, A = ht.A;
  const int ttCap = nextPow2(2 * cap);
  const int rowCap = c.row_capacity > 0 ? c.row_capacity : 4 * G * A;
  if(matchPaths) {
    numNets_ = sharedNet ? 1 : 2;  // a shared net: one instance evaluates both sides
    for(int n = 0; n < numNets_; n++)
      if(matchPaths[n]) {
        nets_[n].model.reset(new ModelHost(loadModel(matchPaths[n])));
        nets_[n].nn.reset(new NNEngine(*nets_[n].model, c.x, c.y, c.win_len, c.nn_precision));
      }
  } else if(!c.use_fake_net) {
    if(!c.model_path)
      throw std::invalid_argument("model_path required unless use_fake_net");
    nets_[0].model.reset(new ModelHost(loadModel(c.model_path)));
    nets_[0].nn.reset(new NNEngine(*nets_[0].model, c.x, c.y, c.win_len, c.nn_precision));
  }
  nnPath_ = c.nn_precision;
  xLen_ = c.x;
  yLen_ = c.y;
  winLen_ = c.win_len;
  SearchDev& d = hd_;
  memset(&d, 0, sizeof(d));
  d.T = T_;
  d.sp = toSP(sp);
  d.spCheap = cheapSearchSP(d.sp);
  d.G = G;
  d.cap = cap;
  d.ttCap = ttCap;
  d.svbCap = ttCap;
  d.P = P;
  d.A = A;
  d.inWords = ht.inWords;
  d.maxTurns = A + 1;
  d.rowCap = rowCap;
  d.slotBase = c.slot_base;
  if(c.start_stagger < 0)
    throw std::invalid_argument("start_stagger must be >= 0");
  d.startStagger = c.start_stagger;
  d.seed = c.seed;
  d.games = devAlloc<GameDev>(owned_, G);
  d.nodes = devAlloc<Node>(owned_, (size_t)G * cap, false);
  d.edges = devAlloc<Edge>(owned_, (size_t)G * cap * INLINE_EDGES, false);
  d.edgePoolCap = edgePoolCapFor(cap, P);
  d.edgePool = devAlloc<Edge>(owned_, (size_t)G * 2 * d.edgePoolCap, false);
  d.policy = devAlloc<float>(owned_, (size_t)G * cap * P, false);
  d.nodeKey = devAlloc<uint64_t>(owned_, (size_t)G * cap * 2, false);
  d.freeList = devAlloc<uint32_t>(owned_, (size_t)G * cap, false);
  d.allocBits = devAlloc<uint32_t>(owned_, (size_t)G * (cap / 32));
  d.ttKey = devAlloc<uint64_t>(owned_, (size_t)G * ttCap * 2, false);
  d.ttNode = devAlloc<int32_t>(owned_, (size_t)G * ttCap, false);
  d.svbKey = devAlloc<uint64_t>(owned_, (size_t)G * 2 * ttCap);
  d.svbD = devAlloc<int64_t>(owned_, (size_t)G * 2 * ttCap);
  d.svbW = devAlloc<int64_t>(owned_, (size_t)G * 2 * ttCap);
  d.accPolicy = devAlloc<float>(owned_, (size_t)G * P);
  d.rawPolicy = devAlloc<float>(owned_, (size_t)G * P);
  d.rootNoised = devAlloc<float>(owned_, (size_t)G * P);
  d.pathNode = devAlloc<int32_t>(owned_, (size_t)G * MAX_DEPTH);
  d.pathSlot = devAlloc<int32_t>(owned_, (size_t)G * MAX_DEPTH);
  d.turns = devAlloc<TurnRec>(owned_, (size_t)G * d.maxTurns);
  d.turnPol = devAlloc<int16_t>(owned_, (size_t)G * d.maxTurns * P);
  d.nnIn = devAlloc<uint64_t>(owned_, (size_t)G * ht.inWords);
  d.nnOut = devAlloc<float>(owned_, (size_t)G * (P + 4));
  d.fin = devAlloc<FinRec>(owned_, G);
  d.fork = devAlloc<ForkRec>(owned_, G);
  d.side = devAlloc<DBoard>(owned_, (size_t)G * MAX_SIDE);
  d.sidePol = devAlloc<int16_t>(owned_, (size_t)G * P);
  d.commitList = devAlloc<int32_t>(owned_, G);
  d.nnTimedEvals = devAlloc<unsigned long long>(owned_, 1);
  d.commitCount = devAlloc<int32_t>(owned_, 1);
  const int pb = (A + 7) / 8;
  d.rBin = devAlloc<uint8_t>(owned_, (size_t)rowCap * NUM_SPATIAL * pb, false);
  d.rGlob = devAlloc<float>(owned_, (size_t)rowCap, false);
  d.rPol = devAlloc<int16_t>(owned_, (size_t)rowCap * 2 * P, false);
  d.rGt = devAlloc<float>(owned_, (size_t)rowCap * 64, false);
  d.rVal = devAlloc<int8_t>(owned_, (size_t)rowCap * 5 * A, false);
  d.rMeta = devAlloc<int32_t>(owned_, (size_t)rowCap * 4, false);
  d.rCount = devAlloc<unsigned long long>(owned_, 1);
  d.rDropped = devAlloc<unsigned long long>(owned_, 1);
  d.rStaged = devAlloc<unsigned long long>(owned_, 1);
  d.nnNeed = devAlloc<int32_t>(owned_, G);
  d.nnDefer = devAlloc<int32_t>(owned_, G);
  d.nnBid = devAlloc<uint32_t>(owned_, G);
  d.nnRR = devAlloc<int32_t>(owned_, 1);
  if(c.nn_batch_cap < 0)
    throw std::invalid_argument("nn_batch_cap must be >= 0");
  if(c.engines_per_device < 0)
    throw std::invalid_argument("engines_per_device must be >= 0");
  userCap_ = c.nn_batch_cap;
  enginesPerDevice_ = std::max(1, c.engines_per_device);
  {
    int dev = 0;
    KC_HIP(hipGetDevice(&dev));
    KC_HIP(hipDeviceGetAttribute(&cus_, hipDeviceAttributeMultiprocessorCount, dev));
    cus_ = std::max(1, cus_);
  }
  d.nnCap = nnCapFor(G);
  d.nnIdx = devAlloc<int32_t>(owned_, G);
  rowsAllocated_ = (size_t)G;
  d.modelGen = devAlloc<int32_t>(owned_, 1);
  d.nnCount = devAlloc<int32_t>(owned_, 1);
  if(c.nn_cache_log2 < 0 || c.nn_cache_log2 > 26)
    throw std::invalid_argument("nn_cache_log2 must be in 0..26");
  d.cacheOn = c.nn_cache_log2 > 0 ? 1 : 0;
  {
    const size_t entries = d.cacheOn ? (size_t)1 << c.nn_cache_log2 : 1;
    d.cacheMask = (uint32_t)(entries - 1);
    d.cKey = devAlloc<uint64_t>(owned_, entries * 2);  // zero key: never a state
    d.cPol = devAlloc<float>(owned_, entries * P, false);
    d.cVal = devAlloc<float>(owned_, entries * 2, false);
    d.cErr = devAlloc<float>(owned_, entries, false);
    d.cTag = devAlloc<uint32_t>(owned_, entries);
    if(matchPaths && !sharedNet) {  // net 1's own cache
      d.cKey1 = devAlloc<uint64_t>(owned_, entries * 2);
      d.cPol1 = devAlloc<float>(owned_, entries * P, false);
      d.cVal1 = devAlloc<float>(owned_, entries * 2, false);
      d.cErr1 = devAlloc<float>(owned_, entries, false);
      d.cTag1 = devAlloc<uint32_t>(owned_, entries);
    }
  }
  if(matchPaths) {
    d.matchMode = 1;
    d.nnIdx1 = devAlloc<int32_t>(owned_, G);
    d.nnCount1 = devAlloc<int32_t>(owned_, 1);
    d.nnPeak = devAlloc<int32_t>(owned_, 2);
    d.nnNetEvals = devAlloc<unsigned long long>(owned_, 2);
    d.matchSharedNet = sharedNet ? 1 : 0;
  }
  {
    coffee_uncertainty_params u;
    coffee_uncertainty_params_default(&u);
    d.unc = toUnc(u);  // off
    d.unc1 = d.unc;
    coffee_exploration_params e;
    coffee_exploration_params_default(&e);
    d.ex = toExpl(e);  // off
    d.ex1 = d.ex;
    d.rs = RootSearch{0.0f, 0.0f};  // off
    d.rs1 = d.rs;
  }
  d.sp1 = d.sp;
  if(perSide) {
    d.matchPerSide = 1;
    d.sp = toSP(matchOpts->side[0].search);
    d.spCheap = cheapSearchSP(d.sp);
    d.sp1 = toSP(matchOpts->side[1].search);
    d.unc = toUnc(matchOpts->side[0].unc);
    d.unc1 = toUnc(matchOpts->side[1].unc);
  }
  d.cClear = devAlloc<uint32_t>(owned_, G);
  d.pendList = devAlloc<int32_t>(owned_, G, false);
  d.pendCount = devAlloc<int32_t>(owned_, 1);
  {
    const char* f = getenv("COFFEE_FUSED_ROUNDS");
    fuseRounds_ = f && f[0] == '0' ? 0 : (f && f[0] == '1' ? 1 : -1);
    const char* r = getenv("COFFEE_SEPARATE_RESOLVE");
    resolveInCompact_ = !(r && r[0] == '1');
  }
  {
    const char* e = getenv("COFFEE_NN_AUDIT_EVERY");
    if(e)
      auditEvery_ = std::max(0, atoi(e));
    const char* t = getenv("COFFEE_NN_AUDIT_TOL");
    if(t)
      auditTol_ = (float)atof(t);
  }
  for(int n = 0; n < numNets_; n++) {
    nets_[n].auditOut = devAlloc<float>(owned_, (size_t)G * (P + 4), false);
    nets_[n].auditMax = devAlloc<unsigned>(owned_, 1);
  }
  d.gCap = 2 * G;
  d.gRec = devAlloc<GameRec>(owned_, (size_t)d.gCap, false);
  d.gCount = devAlloc<unsigned long long>(owned_, 1);
  d.gDropped = devAlloc<unsigned long long>(owned_, 1);
  d.spGames = devAlloc<unsigned long long>(owned_, 1);  // no start-position table: spN 0
  dd_ = devAlloc<SearchDev>(owned_, 1);
  KC_HIP(hipMemcpy(dd_, &d, sizeof(SearchDev), hipMemcpyHostToDevice));
  KC_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  const size_t lds = commitLdsBytes(cap);
  if(lds > 64 * 1024)
    throw std::invalid_argument("node_cap too large for the commit kernel's LDS");
  launchSelfplayInit(d, dd_, stream_);
  KC_HIP(hipStreamSynchronize(stream_));
}

SelfplayEngine::~SelfplayEngine() {
  if(stream_)
    (void)hipStreamSynchronize(stream_);
  for(const PendingTiming& p : pending_) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  for(hipEvent_t e : evPool_)
    (void)hipEventDestroy(e);
  for(Net& n : nets_)
    n.nn.reset();
  for(void* p : owned_)
    (void)hipFree(p);
  if(hd_.spTable.p)
    (void)hipFree(const_cast<coffee_start_position*>(hd_.spTable.p));
  if(hd_.spCum.p)
    (void)hipFree(const_cast<uint64_t*>(hd_.spCum.p));
  if(stream_)
    (void)hipStreamDestroy(stream_);
}

// Kernel timing: an event pair per launch on the launch stream, resolved later
// (no host synchronisation inside the round loop).
hipEvent_t SelfplayEngine::takeEvent() {
  if(evPool_.empty()) {
    hipEvent_t e;
    KC_HIP(hipEventCreate(&e));
    return e;
  }
  hipEvent_t e = evPool_.back();
  evPool_.pop_back();
  return e;
}

void SelfplayEngine::timed(int which, hipStream_t st, const std::function<void()>& f, bool on) {
  if(!on) {
    f();
    return;
  }
  hipEvent_t a = takeEvent(), b = takeEvent();
  KC_HIP(hipEventRecord(a, st));
  f();
  KC_HIP(hipEventRecord(b, st));
  pending_.push_back({which, a, b});
}

void SelfplayEngine::timedKernel(int which, bool on, const std::function<void(hipEvent_t, hipEvent_t)>& f) {
  if(!on) {
    f(nullptr, nullptr);
    return;
  }
  hipEvent_t a = takeEvent(), b = takeEvent();
  f(a, b);
  pending_.push_back({which, a, b});
}

void SelfplayEngine::resolveTiming() {
  for(const PendingTiming& p : pending_) {
    KC_HIP(hipEventSynchronize(p.b));
    float ms = 0.0f;
    KC_HIP(hipEventElapsedTime(&ms, p.a, p.b));
    kernelMs_[p.which] += ms;
    kernelLaunches_[p.which]++;
    evPool_.push_back(p.a);
    evPool_.push_back(p.b);
  }
  pending_.clear();
}

bool SelfplayEngine::fuseNow() const {
  // match play and parallel playouts always run the separate select and backup kernels
  if(hd_.matchMode || hd_.wideK > 1)
    return false;
  if(fuseRounds_ >= 0)
    return fuseRounds_ == 1;
  const std::unique_ptr<NNEngine>& nn = nets_[0].nn;
  return !nn || (nn->fused() && nn->precision() == NN_FAST);
}

void SelfplayEngine::step(int rounds, hipStream_t st) {
  if(!st)
    st = stream_;
  const SearchDev& d = hd_;
  const bool fuse = fuseNow();
  bool selected = false;  // this round's selections ran in the previous round's fused kernel
  // analysis: the idle slots take the queries submitted since the last step (the report
  // part of the launch finds nothing new).  Also with rounds == 0: queries that need no
  // search are then answered without a round
  if(d.analysisMode) {
    hd_.aSubmitted = aSubmitted_;
    launchCommit(d, dd_, st);
  }
  for(int r = 0; r < rounds; r++) {
    const bool t1 = sampleNow(1);
    // select, network and backup are timed by their own dispatches (kernel start to
    // end, like rocprofv3); compact and cache write run untimed between them
    if(selected) {
      if(!resolveInCompact_)
        launchResolve(d, dd_, st);  // the selections whose cache slot was being written
    } else {
      const bool t0 = sampleNow(0);
      timedKernel(0, t0, [&](hipEvent_t a, hipEvent_t b) { launchSelect(d, dd_, st, a, b, commitReset_); });
    }
    commitReset_ = false;
    launchCompact(d, dd_, st, t1, selected && resolveInCompact_);
    timedKernel(1, t1, [&](hipEvent_t a, hipEvent_t b) { forwardNet(0, d.nnCount, d.nnIdx, st, a, b); });
    // match play: net 1's list in its own launch, after net 0's on the same stream
    // (a shared net evaluates both sides' rows in the launch above)
    if(d.matchMode && !d.matchSharedNet)
      forwardNet(1, d.nnCount1, d.nnIdx1, st, nullptr, nullptr);
    const bool commitNow = (rounds_ + 1) % (uint64_t)commitInterval_ == 0 || r == rounds - 1;
    if(fuse && !commitNow) {
      const bool t4 = sampleNow(4);
      timedKernel(4, t4, [&](hipEvent_t a, hipEvent_t b) { launchBackupSelect(d, dd_, st, a, b); });
      selected = true;
    } else {
      const bool t2 = sampleNow(2);
      timedKernel(2, t2, [&](hipEvent_t a, hipEvent_t b) { launchBackup(d, dd_, st, a, b); });
      selected = false;
    }
    rounds_++;
    if(commitNow) {
      const bool t3 = sampleNow(3);
      timed(3, st, [&] { launchCommit(d, dd_, st); }, t3);
      commitReset_ = true;  // the next kSelect zeroes the count (no separate memset)
    }
  }
}

void SelfplayEngine::setUncertainty(const coffee_uncertainty_params& p) {
  const Unc u = toUnc(p);
  if(hd_.matchPerSide)
    throw std::invalid_argument("set_uncertainty: the match engine's sides carry their own (coffee_match_options)");
  // a tree must never mix the two rules: only before the first round, and in analysis before
  // the first query (a step loads the queued queries, also one of zero rounds)
  if(rounds_ > 0 || aSubmitted_ > 0)
    throw std::invalid_argument(hd_.analysisMode ? "set_uncertainty: only before the first query and round"
                                                 : "set_uncertainty: only before the engine's first round");
  hd_.unc = u;
  // nothing runs yet (the constructor synchronised its initialisation): a plain copy
  KC_HIP(hipMemcpy(&dd_->unc, &hd_.unc, sizeof(Unc), hipMemcpyHostToDevice));
}

void SelfplayEngine::setExploration(int side, const coffee_exploration_params& p) {
  const Expl e = toExpl(p);
  if(hd_.matchPerSide ? (side != 0 && side != 1) : side != -1)
    throw std::invalid_argument(hd_.matchPerSide ? "set_exploration: side must be 0 or 1 on an engine with per-side settings"
                                                 : "set_exploration: side must be -1 on an engine without per-side settings");
  // like set_uncertainty: a tree must never mix the two rules
  if(rounds_ > 0 || aSubmitted_ > 0)
    throw std::invalid_argument(hd_.analysisMode ? "set_exploration: only before the first query and round"
                                                 : "set_exploration: only before the engine's first round");
  if(side != 1)
    hd_.ex = e;
  if(side != 0)
    hd_.ex1 = e;
  // nothing runs yet (the constructor synchronised its initialisation): plain copies
  KC_HIP(hipMemcpy(&dd_->ex, &hd_.ex, sizeof(Expl), hipMemcpyHostToDevice));
  KC_HIP(hipMemcpy(&dd_->ex1, &hd_.ex1, sizeof(Expl), hipMemcpyHostToDevice));
}

void SelfplayEngine::setRootSearch(int side, const coffee_root_search_params& p) {
  const RootSearch r = toRootSearch(p);
  if(hd_.matchPerSide ? (side != 0 && side != 1) : side != -1)
    throw std::invalid_argument(hd_.matchPerSide ? "set_root_search: side must be 0 or 1 on an engine with per-side settings"
                                                 : "set_root_search: side must be -1 on an engine without per-side settings");
  // like set_exploration: a tree must never mix the two rules
  if(rounds_ > 0 || aSubmitted_ > 0)
    throw std::invalid_argument(hd_.analysisMode ? "set_root_search: only before the first query and round"
                                                 : "set_root_search: only before the engine's first round");
  if(side != 1)
    hd_.rs = r;
  if(side != 0)
    hd_.rs1 = r;
  // nothing runs yet (the constructor synchronised its initialisation): plain copies
  KC_HIP(hipMemcpy(&dd_->rs, &hd_.rs, sizeof(RootSearch), hipMemcpyHostToDevice));
  KC_HIP(hipMemcpy(&dd_->rs1, &hd_.rs1, sizeof(RootSearch), hipMemcpyHostToDevice));
}

void SelfplayEngine::setRootOptions(const coffee_analysis_root_options& o) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  if((o.root_symmetry_pruning != 0 && o.root_symmetry_pruning != 1) || (o.include_policy != 0 && o.include_policy != 1))
    throw std::invalid_argument("set_root_options: root_symmetry_pruning and include_policy must be 0 or 1");
  // a query's mask is computed when a slot loads it: only before the first query
  if(aSubmitted_ > 0)
    throw std::invalid_argument("set_root_options: only before the first query");
  hd_.aPrune = o.root_symmetry_pruning;
  if(o.include_policy && hd_.aPolicy.p == nullptr)
    hd_.aPolicy = devAlloc<float>(owned_, (size_t)hd_.aCap * hd_.P);
  aIncludePolicy_ = o.include_policy != 0;
  // nothing runs yet (the constructor synchronised its initialisation): a plain copy.  A policy
  // ring allocated by an earlier call stays allocated; the kernels see it only while asked for
  SearchDev dev = hd_;
  if(!aIncludePolicy_)
    dev.aPolicy = nullptr;
  KC_HIP(hipMemcpy(&dd_->aPrune, &dev.aPrune, sizeof(int32_t), hipMemcpyHostToDevice));
  KC_HIP(hipMemcpy(&dd_->aPolicy, &dev.aPolicy, sizeof(dev.aPolicy), hipMemcpyHostToDevice));
}

void validateAnalysisRestrict(int x, int y, uint64_t id, const coffee_analysis_restrict& r) {
  const int P = 4 * x * y;
  const std::string who = "analysis query " + std::to_string(id);
  if(r.mode < RM_NONE || r.mode > RM_ALLOW)
    throw std::invalid_argument(who + ": restrict mode must be 0 (none), 1 (avoid) or 2 (allow)");
  if(r.mode == RM_NONE)
    return;
  if(P > 32 * RM_QUERY_WORDS)
    throw std::invalid_argument(who + ": avoid / allow sets need a board of at most " +
                                std::to_string(32 * RM_QUERY_WORDS) + " positions");
  if(rmBitsPastP(P, r.avoid))
    throw std::invalid_argument(who + ": avoid / allow bit at a position >= " + std::to_string(P));
}

// ---- start positions (startpos.h) ----

void validateStartPosParams(const coffee_start_positions_params& p) {
  // the reference's getters (play.cpp:190-196, setup / PlaySettings); NaN is out of range
  auto in = [](float x, float lo, float hi) { return x >= lo && x <= hi; };
  if(!in(p.prob, 0.0f, 1.0f))
    throw std::invalid_argument("start positions: prob must be in [0, 1]");
  if(!in(p.turn_weight_lambda, -10.0f, 10.0f))
    throw std::invalid_argument("start positions: turn_weight_lambda must be in [-10, 10]");
  if(!in(p.start_policy_init_area_prop, 0.0f, 1.0f))
    throw std::invalid_argument("start positions: start_policy_init_area_prop must be in [0, 1]");
}

void startPosThresholdsOf(const coffee_start_position* samples, int n, float lambda, uint64_t* cum) {
  if(n < 1 || !samples || !cum)
    throw std::invalid_argument("start positions: the table needs at least one sample");
  if(!(lambda >= -10.0f && lambda <= 10.0f))
    throw std::invalid_argument("start positions: turn_weight_lambda must be in [-10, 10]");
  std::vector<float> w(n);
  std::vector<int32_t> t(n);
  for(int i = 0; i < n; i++) {
    w[i] = samples[i].weight;
    t[i] = samples[i].num_moves;
    if(!(w[i] >= 0.0f) || !std::isfinite(w[i]))
      throw std::invalid_argument("start position " + std::to_string(i) + ": weight must be finite and >= 0");
    if(!std::isfinite(std::exp(-(double)t[i] * (double)lambda) * (double)w[i]))
      throw std::invalid_argument("start position " + std::to_string(i) + ": weight * exp(-num_moves * lambda) is " +
                                  "not finite (num_moves " + std::to_string(t[i]) + ")");
  }
  // what is left for the builder to refuse: no sample with a positive probability, or a sum past double
  if(!startPosThresholds(w.data(), t.data(), n, (double)lambda, cum))
    throw std::invalid_argument("start positions: no sample has a positive probability (or their sum is not finite)");
}

// The check kernel on samples already on the device (st: any stream; synchronised here).
static void checkStartPosDevice(const DTables* T, int P, const coffee_start_position* dev, int n, int32_t* status,
                                int32_t* info, hipStream_t st) {
  std::vector<void*> tmp;
  struct Free {
    std::vector<void*>& t;
    ~Free() {
      for(void* p : t)
        (void)hipFree(p);
    }
  } guard{tmp};
  // (weak in search.h: a host-only link of the engine has no kernels; never null in the library)
  if(!launchStartPosCheck)
    throw InternalError("start positions: this build has no check kernel");
  int32_t* ds = devAlloc<int32_t>(tmp, (size_t)n, false);
  int32_t* di = devAlloc<int32_t>(tmp, (size_t)n, false);
  KC_HIP(hipMemsetAsync(ds, 0xFF, sizeof(int32_t) * n, st));
  KC_HIP(hipMemsetAsync(di, 0, sizeof(int32_t) * n, st));
  launchStartPosCheck(T, P, dev, n, ds, di, st);
  KC_HIP(hipStreamSynchronize(st));
  KC_HIP(hipMemcpy(status, ds, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  KC_HIP(hipMemcpy(info, di, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
}

void checkStartPositions(int x, int y, int winLen, int n, const coffee_start_position* samples, int32_t* status,
                         int32_t* info) {
  if(n < 0 || (n > 0 && (!samples || !status || !info)))
    throw std::invalid_argument("start positions: NULL argument or n < 0");
  if(n == 0)
    return;
  const DTables* T = deviceTables(x, y, winLen);
  coffee_start_position* dev = nullptr;
  KC_HIP(hipMalloc(&dev, sizeof(coffee_start_position) * (size_t)n));
  try {
    KC_HIP(hipMemcpy(dev, samples, sizeof(coffee_start_position) * (size_t)n, hipMemcpyHostToDevice));
    checkStartPosDevice(T, 4 * x * y, dev, n, status, info, nullptr);
  } catch(...) {
    (void)hipFree(dev);
    throw;
  }
  KC_HIP(hipFree(dev));
}

void SelfplayEngine::setStartPositions(const coffee_start_position* samples, int n,
                                       const coffee_start_positions_params& p) {
  if(hd_.analysisMode)
    throw std::invalid_argument("start positions: not for an analysis engine");
  validateStartPosParams(p);
  if(n < 0 || (n > 0 && !samples))
    throw std::invalid_argument("start positions: NULL table or n < 0");
  coffee_start_position* table = nullptr;
  uint64_t* cumDev = nullptr;
  if(n > 0) {
    // host part first: weights and thresholds; then the replay of every sample on the device,
    // into buffers of its own -- the engine's state is untouched until the table is accepted
    std::vector<uint64_t> cum(n);
    startPosThresholdsOf(samples, n, p.turn_weight_lambda, cum.data());
    std::vector<int32_t> status(n), info(n);
    KC_HIP(hipMalloc(&table, sizeof(coffee_start_position) * (size_t)n));
    try {
      // (blocking copies into buffers no kernel reads yet; the check itself runs on the engine stream)
      KC_HIP(hipMemcpy(table, samples, sizeof(coffee_start_position) * (size_t)n, hipMemcpyHostToDevice));
      checkStartPosDevice(T_, hd_.P, table, n, status.data(), info.data(), stream_);
      for(int i = 0; i < n; i++)
        if(status[i] != COFFEE_ANALYSIS_OK) {
          static const char* const what[] = {"", "illegal move at index ", "the moves end the game, winner ",
                                             "no legal move"};
          std::string m = "start position " + std::to_string(i) + ": " + what[status[i] & 3];
          if(status[i] != COFFEE_ANALYSIS_NO_LEGAL_MOVE)
            m += std::to_string(info[i]);
          throw std::invalid_argument(m);
        }
      KC_HIP(hipMalloc(&cumDev, sizeof(uint64_t) * (size_t)n));
      KC_HIP(hipMemcpy(cumDev, cum.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
    } catch(...) {
      (void)hipFree(table);
      (void)hipFree(cumDev);
      throw;
    }
  }
  sync();  // nothing of the engine runs while the table changes hands
  coffee_start_position* oldTable = const_cast<coffee_start_position*>(hd_.spTable.p);
  uint64_t* oldCum = const_cast<uint64_t*>(hd_.spCum.p);
  hd_.spTable = table;
  hd_.spCum = cumDev;
  hd_.spN = n;
  hd_.spProb = n > 0 ? p.prob : 0.0f;
  hd_.spInitAreaProp = p.start_policy_init_area_prop;
  // the start-position fields are the tail of SearchDev; the engine stream is idle (sync above),
  // so a plain copy is ordered before the next launch on it
  const size_t off = (size_t)((const char*)&hd_.spTable - (const char*)&hd_);
  KC_HIP(hipMemcpy((char*)dd_ + off, (const char*)&hd_ + off, sizeof(SearchDev) - off, hipMemcpyHostToDevice));
  if(rounds_ == 0) {
    // no round ran yet: every slot's first game starts again, now with the table
    KC_HIP(hipMemsetAsync(hd_.spGames, 0, sizeof(unsigned long long), stream_));
    launchSelfplayInit(hd_, dd_, stream_);
  }
  KC_HIP(hipStreamSynchronize(stream_));
  if(oldTable)
    (void)hipFree(oldTable);
  if(oldCum)
    (void)hipFree(oldCum);
}

uint64_t SelfplayEngine::startPositionGames() {
  sync();
  unsigned long long v = 0;
  KC_HIP(hipMemcpy(&v, hd_.spGames, 8, hipMemcpyDeviceToHost));
  return v;
}

void SelfplayEngine::forwardNet(int n, const int32_t* count, const int32_t* idx, hipStream_t st, hipEvent_t a,
                                hipEvent_t b) {
  const SearchDev& d = hd_;
  Net& net = nets_[n];
  const int rows = std::min(this->rows(), d.nnCap);  // grid bound; the batch is *count rows
  if(net.nn) {
    net.nn->forward(rows, d.nnIn, d.nnOut, st, count, idx, a, b);
  } else {
    if(a)
      KC_HIP(hipEventRecord(a, st));
    launchFakeNet(T_, rows, d.nnIn, d.nnOut, st, count, idx);
    if(b)
      KC_HIP(hipEventRecord(b, st));
  }
  if(net.nn && nnPath_ == NN_DEFAULT && auditEvery_ > 0 && net.nn->precision() == NN_CORRECTED &&
     net.nnLaunches++ % (uint64_t)auditEvery_ == 0) {
    net.nn->audit(rows, d.nnIn, d.nnOut, net.auditOut, net.auditMax, st, count, idx);
    net.audits++;
  }
}

void SelfplayEngine::sync() {
  KC_HIP(hipStreamSynchronize(stream_));
  resolveTiming();
  auditCheck();
}

void SelfplayEngine::auditCheck() {
  for(int n = 0; n < numNets_; n++) {
    Net& net = nets_[n];
    if(!net.nn || net.audits == 0)
      continue;
    unsigned bits = 0;
    KC_HIP(hipMemcpy(&bits, net.auditMax, 4, hipMemcpyDeviceToHost));
    float m;
    memcpy(&m, &bits, 4);
    net.auditSeen = std::max(net.auditSeen, m);
    if(!(net.auditSeen <= auditTol_) && net.nn->precision() == NN_CORRECTED && nnPath_ == NN_DEFAULT) {
      // the corrected instance missed the default precision's bound on self-play positions:
      // the same model on the accurate instance from here on (this net's cached evaluations cleared)
      net.nn.reset(new NNEngine(*net.model, xLen_, yLen_, winLen_, NN_ACCURATE));
      net.auditSwitches++;
      const int cap = nnCapFor(rows());
      if(cap != hd_.nnCap) {
        hd_.nnCap = cap;
        KC_HIP(hipMemcpy(&dd_->nnCap, &cap, sizeof(int), hipMemcpyHostToDevice));
      }
      if(hd_.cacheOn)
        KC_HIP(hipMemsetAsync(n ? hd_.cKey1 : hd_.cKey, 0, sizeof(uint64_t) * 2 * ((size_t)hd_.cacheMask + 1),
                              stream_));
      KC_HIP(hipStreamSynchronize(stream_));
    }
  }
}

void SelfplayEngine::stats(coffee_selfplay_stats& out) {
  sync();
  std::vector<GameDev> g(hd_.G);
  KC_HIP(hipMemcpy(g.data(), hd_.games, sizeof(GameDev) * hd_.G, hipMemcpyDeviceToHost));
  memset(&out, 0, sizeof(out));
  out.rounds = rounds_;
  for(const GameDev& x : g) {
    out.playouts += x.playouts;
    out.nn_evals += x.nnEvals;
    out.moves += x.moves;
    out.games_finished += x.gamesFinished;
    out.errors += x.err != 0 ? 1 : 0;
    out.errors_node_pool += x.err == ERR_NODE_POOL ? 1 : 0;
    out.errors_edge_pool += x.err == ERR_EDGE_POOL ? 1 : 0;
    out.edge_pool_peak = std::max<uint64_t>(out.edge_pool_peak, (uint64_t)x.edgePeak);
    out.tree_levels += x.treeLevels;
    out.tree_children += x.treeChildren;
  }
  unsigned long long cnt = 0, dropped = 0;
  KC_HIP(hipMemcpy(&cnt, hd_.rCount, 8, hipMemcpyDeviceToHost));
  KC_HIP(hipMemcpy(&dropped, hd_.rDropped, 8, hipMemcpyDeviceToHost));
  unsigned long long staged = 0;
  KC_HIP(hipMemcpy(&staged, hd_.rStaged, 8, hipMemcpyDeviceToHost));
  out.rows_pending = cnt;
  out.rows_written = rowsDrained_ + staged + cnt;
  out.rows_dropped = dropped;
  unsigned long long gdrop = 0;
  KC_HIP(hipMemcpy(&gdrop, hd_.gDropped, 8, hipMemcpyDeviceToHost));
  out.games_dropped = gdrop;
  out.edge_pool_cap = (uint64_t)hd_.edgePoolCap;
  out.nn_precision = nets_[0].nn ? (uint64_t)nets_[0].nn->precision() : 0;
  out.nn_audits = nets_[0].audits;
  out.nn_audit_switches = (uint64_t)nets_[0].auditSwitches;
  out.nn_audit_max_diff = nets_[0].auditSeen;
  if(out.errors)
    throw InternalError("self-play device invariant violated in " + std::to_string(out.errors) +
                        " game slot(s): " + std::to_string(out.errors_node_pool) + " node pool exhausted, " +
                        std::to_string(out.errors_edge_pool) + " edge pool exhausted, " +
                        std::to_string(out.errors - out.errors_node_pool - out.errors_edge_pool) +
                        " without a move candidate (raise node_cap)");
}

void SelfplayEngine::matchStats(coffee_match_stats& out) {
  if(!hd_.matchMode)
    throw std::invalid_argument("not a match engine");
  coffee_selfplay_stats s;
  stats(s);  // throws on a device error, as for self-play
  memset(&out, 0, sizeof(out));
  out.rounds = s.rounds;
  out.playouts = s.playouts;
  out.moves = s.moves;
  out.games_finished = s.games_finished;
  out.games_dropped = s.games_dropped;
  out.errors = s.errors;
  // evaluations per net: the rows kCompact listed for the two launches (the games' own
  // counters do not say which net answered)
  int32_t peak[2] = {0, 0};
  unsigned long long evals[2] = {0, 0};
  KC_HIP(hipMemcpy(peak, hd_.nnPeak, sizeof(peak), hipMemcpyDeviceToHost));
  KC_HIP(hipMemcpy(evals, hd_.nnNetEvals, sizeof(evals), hipMemcpyDeviceToHost));
  for(int n = 0; n < 2; n++) {
    out.nn_evals[n] = evals[n];
    out.nn_batch_peak[n] = (uint64_t)peak[n];
    out.nn_precision[n] = nets_[n].nn ? (uint64_t)nets_[n].nn->precision() : 0;
    out.nn_audits[n] = nets_[n].audits;
    out.nn_audit_switches[n] = (uint64_t)nets_[n].auditSwitches;
    out.nn_audit_max_diff[n] = nets_[n].auditSeen;
  }
}

int SelfplayEngine::analysisSubmit(const coffee_analysis_query* q, const coffee_analysis_restrict* rs, int n) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  for(int i = 0; i < n; i++) {
    validateAnalysisQuery(xLen_, yLen_, q[i]);
    if(q[i].max_visits > hd_.cap - 4)
      throw std::invalid_argument("analysis query " + std::to_string(q[i].id) + ": max_visits must be <= node_cap - 4 (" +
                                  std::to_string(hd_.cap - 4) + ")");
    if(rs)
      validateAnalysisRestrict(xLen_, yLen_, q[i].id, rs[i]);
  }
  const uint64_t cap = (uint64_t)hd_.aCap;
  const int take = (int)std::min<uint64_t>((uint64_t)std::max(n, 0), cap - (aSubmitted_ - aDrained_));
  // The ring entries [first, first + take) mod cap, in at most two contiguous copies.  They
  // are free: the queries they held were drained.  The copies return when the data is on the
  // device and do not wait for the engine stream; kernels learn of the new entries only from
  // the submitted count, which the next step's first launch carries.
  const uint64_t first = aSubmitted_ % cap;
  const uint64_t run0 = std::min<uint64_t>((uint64_t)take, cap - first);
  if(run0 > 0)
    KC_HIP(hipMemcpy(hd_.aQuery + first, q, sizeof(coffee_analysis_query) * run0, hipMemcpyHostToDevice));
  if((uint64_t)take > run0)
    KC_HIP(hipMemcpy(hd_.aQuery, q + run0, sizeof(coffee_analysis_query) * ((uint64_t)take - run0),
                     hipMemcpyHostToDevice));
  // the restrictions beside them (none given: zeroed entries, mode 0)
  std::vector<coffee_analysis_restrict> none;
  if(!rs && take > 0) {
    none.assign((size_t)take, coffee_analysis_restrict{});
    rs = none.data();
  }
  coffee_analysis_restrict* ring = const_cast<coffee_analysis_restrict*>(hd_.aRestrict.p);
  if(run0 > 0)
    KC_HIP(hipMemcpy(ring + first, rs, sizeof(coffee_analysis_restrict) * run0, hipMemcpyHostToDevice));
  if((uint64_t)take > run0)
    KC_HIP(hipMemcpy(ring, rs + run0, sizeof(coffee_analysis_restrict) * ((uint64_t)take - run0),
                     hipMemcpyHostToDevice));
  aSubmitted_ += (uint64_t)take;
  return take;
}

int SelfplayEngine::analysisDrain(int max, coffee_analysis_result* header, coffee_analysis_move* moves,
                                  coffee_analysis_root_info* rootInfo, float* policy) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  if(policy && !aIncludePolicy_)
    throw std::invalid_argument("policy_out: the engine was not set to include_policy (coffee_analysis_set_root_options)");
  sync();
  unsigned long long written = 0;
  KC_HIP(hipMemcpy(&written, hd_.aCtr + AC_RESULTS, 8, hipMemcpyDeviceToHost));
  const uint64_t cap = (uint64_t)hd_.aCap, P = (uint64_t)hd_.P;
  const int n = (int)std::min<uint64_t>(written - aDrained_, (uint64_t)std::max(max, 0));
  if(n > 0 && !header)
    throw std::invalid_argument("header_out is NULL");
  const uint64_t first = aDrained_ % cap;
  const uint64_t run0 = std::min<uint64_t>((uint64_t)n, cap - first), run1 = (uint64_t)n - run0;
  if(run0 > 0) {
    KC_HIP(hipMemcpy(header, hd_.aRes + first, sizeof(coffee_analysis_result) * run0, hipMemcpyDeviceToHost));
    if(moves)
      KC_HIP(hipMemcpy(moves, hd_.aMoves + first * P, sizeof(coffee_analysis_move) * P * run0, hipMemcpyDeviceToHost));
    if(rootInfo)
      KC_HIP(hipMemcpy(rootInfo, hd_.aRootInfo + first, sizeof(coffee_analysis_root_info) * run0, hipMemcpyDeviceToHost));
    if(policy)
      KC_HIP(hipMemcpy(policy, hd_.aPolicy + first * P, sizeof(float) * P * run0, hipMemcpyDeviceToHost));
  }
  if(run1 > 0) {
    KC_HIP(hipMemcpy(header + run0, hd_.aRes, sizeof(coffee_analysis_result) * run1, hipMemcpyDeviceToHost));
    if(moves)
      KC_HIP(hipMemcpy(moves + run0 * P, hd_.aMoves, sizeof(coffee_analysis_move) * P * run1, hipMemcpyDeviceToHost));
    if(rootInfo)
      KC_HIP(hipMemcpy(rootInfo + run0, hd_.aRootInfo, sizeof(coffee_analysis_root_info) * run1, hipMemcpyDeviceToHost));
    if(policy)
      KC_HIP(hipMemcpy(policy + run0 * P, hd_.aPolicy, sizeof(float) * P * run1, hipMemcpyDeviceToHost));
  }
  // a ring entry's records past its children belong to earlier results
  if(moves)
    for(int i = 0; i < n; i++) {
      const uint64_t k = (uint64_t)std::min<int64_t>(std::max<int64_t>(header[i].num_children, 0), (int64_t)P);
      memset(moves + (uint64_t)i * P + k, 0, sizeof(coffee_analysis_move) * (P - k));
    }
  // ... and so does the policy row of a result without a search
  if(policy)
    for(int i = 0; i < n; i++)
      if(header[i].status != COFFEE_ANALYSIS_OK)
        memset(policy + (uint64_t)i * P, 0, sizeof(float) * P);
  aDrained_ += (uint64_t)n;
  return n;
}

void SelfplayEngine::setSearchThreads(int threads, float perThread) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  if(threads < 1 || threads > MAX_SEARCH_THREADS)
    throw std::invalid_argument("set_search_threads: threads must be in 1.." + std::to_string(MAX_SEARCH_THREADS));
  if(!(perThread > 0.0f) || !std::isfinite(perThread))
    throw std::invalid_argument("set_search_threads: virtual_losses_per_thread must be finite and > 0");
  // a tree never mixes two settings: every submitted query has its result
  sync();
  unsigned long long written = 0;
  KC_HIP(hipMemcpy(&written, hd_.aCtr + AC_RESULTS, 8, hipMemcpyDeviceToHost));
  if(written != aSubmitted_)
    throw std::invalid_argument("set_search_threads: only while the engine holds no query");
  // a wide round fits one network launch: no row is ever deferred
  const size_t rows = (size_t)hd_.G * threads;
  if(threads > 1) {
    const int cap = nnCapFor(1 << 30);
    if(rows > (size_t)cap)
      throw std::invalid_argument("set_search_threads: num_slots x threads = " + std::to_string(rows) +
                                  " exceeds the batch cap of one network launch (" + std::to_string(cap) + ")");
  }
  SearchDev& d = hd_;
  if(rows > rowsAllocated_) {
    // the network batch arrays by row; the ones they replace stay owned until the engine goes
    d.nnIn = devAlloc<uint64_t>(owned_, rows * d.inWords);
    d.nnOut = devAlloc<float>(owned_, rows * (d.P + 4));
    d.nnNeed = devAlloc<int32_t>(owned_, rows);
    d.nnBid = devAlloc<uint32_t>(owned_, rows);
    d.nnIdx = devAlloc<int32_t>(owned_, rows);
    for(int n = 0; n < numNets_; n++)
      nets_[n].auditOut = devAlloc<float>(owned_, rows * (d.P + 4), false);
    d.wideRec = devAlloc<WideRec>(owned_, rows);
    d.widePathNode = devAlloc<int32_t>(owned_, rows * MAX_DEPTH);
    d.widePathSlot = devAlloc<int32_t>(owned_, rows * MAX_DEPTH);
    if(d.wideCount.p == nullptr) {
      d.wideCount = devAlloc<int32_t>(owned_, d.G);
      d.wideCtr = devAlloc<unsigned long long>(owned_, WC_N);
    }
    rowsAllocated_ = rows;
  }
  d.wideK = threads;
  d.vlPerThread = perThread;
  d.nnCap = nnCapFor((int)rows);
  // the stream is idle (sync above): plain copies, member by member (the device copy's aPolicy
  // may differ from the host's, setRootOptions)
  auto up = [&](auto SearchDev::*m) {
    KC_HIP(hipMemcpy(&(dd_->*m), &(d.*m), sizeof(d.*m), hipMemcpyHostToDevice));
  };
  up(&SearchDev::nnIn);
  up(&SearchDev::nnOut);
  up(&SearchDev::nnNeed);
  up(&SearchDev::nnBid);
  up(&SearchDev::nnIdx);
  up(&SearchDev::nnCap);
  up(&SearchDev::wideRec);
  up(&SearchDev::widePathNode);
  up(&SearchDev::widePathSlot);
  up(&SearchDev::wideCount);
  up(&SearchDev::wideCtr);
  up(&SearchDev::wideK);
  up(&SearchDev::vlPerThread);
}

void SelfplayEngine::searchThreadsInfo(coffee_search_threads_info& out) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  sync();
  memset(&out, 0, sizeof(out));
  out.threads = std::max(1, (int)hd_.wideK);
  out.virtual_losses_per_thread = hd_.wideK >= 1 ? hd_.vlPerThread : 1.0f;
  if(hd_.wideCtr.p != nullptr) {
    unsigned long long c[WC_N];
    KC_HIP(hipMemcpy(c, hd_.wideCtr, sizeof(c), hipMemcpyDeviceToHost));
    out.descents = c[WC_DESCENTS];
    out.collisions = c[WC_COLLISIONS];
  }
  if(!launchVirtualLossCount)
    throw std::runtime_error("search_threads_info: the search kernels are not linked");
  if(!vlCount_)
    vlCount_ = devAlloc<unsigned long long>(owned_, 1);
  launchVirtualLossCount(hd_, dd_, vlCount_, stream_);
  KC_HIP(hipStreamSynchronize(stream_));
  unsigned long long live = 0;
  KC_HIP(hipMemcpy(&live, vlCount_, 8, hipMemcpyDeviceToHost));
  out.live_virtual_losses = live;
}

void SelfplayEngine::roundPaths(int slot, coffee_round_paths& out) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  if(slot < 0 || slot >= hd_.G)
    throw std::invalid_argument("slot out of range");
  sync();
  memset(&out, 0, sizeof(out));
  if(hd_.wideK <= 1)
    return;
  const int K = hd_.wideK;
  int32_t made = 0;
  KC_HIP(hipMemcpy(&made, hd_.wideCount + slot, 4, hipMemcpyDeviceToHost));
  made = std::min(std::max(made, 0), K);
  std::vector<WideRec> rec((size_t)K);
  std::vector<int32_t> pn((size_t)K * MAX_DEPTH), ps((size_t)K * MAX_DEPTH);
  const size_t row0 = (size_t)slot * K;
  KC_HIP(hipMemcpy(rec.data(), hd_.wideRec + row0, sizeof(WideRec) * K, hipMemcpyDeviceToHost));
  KC_HIP(hipMemcpy(pn.data(), hd_.widePathNode + row0 * MAX_DEPTH, 4 * (size_t)K * MAX_DEPTH, hipMemcpyDeviceToHost));
  KC_HIP(hipMemcpy(ps.data(), hd_.widePathSlot + row0 * MAX_DEPTH, 4 * (size_t)K * MAX_DEPTH, hipMemcpyDeviceToHost));
  static_assert(COFFEE_ROUND_PATH_MAX == MAX_DEPTH && COFFEE_SEARCH_THREADS_MAX == MAX_SEARCH_THREADS,
                "katacoffee.h path geometry");
  out.num_descents = made;
  for(int j = 0; j < made; j++) {
    coffee_round_path& o = out.path[j];
    o.leaf_kind = rec[j].leafKind;
    o.path_len = std::min(std::max(rec[j].pathLen, 0), MAX_DEPTH);
    const int n = std::min(MAX_DEPTH, o.path_len + (o.leaf_kind == LEAF_COLLISION ? 1 : 0));
    for(int i = 0; i < n; i++) {
      o.node[i] = pn[(size_t)j * MAX_DEPTH + i];
      o.child_slot[i] = ps[(size_t)j * MAX_DEPTH + i];
    }
  }
}

void SelfplayEngine::analysisStats(coffee_analysis_stats& out) {
  if(!hd_.analysisMode)
    throw std::invalid_argument("not an analysis engine");
  coffee_selfplay_stats s;
  stats(s);  // throws on a device error, as for self-play
  unsigned long long c[AC_N];
  KC_HIP(hipMemcpy(c, hd_.aCtr, sizeof(c), hipMemcpyDeviceToHost));
  memset(&out, 0, sizeof(out));
  out.rounds = s.rounds;
  out.playouts = s.playouts;
  out.nn_evals = s.nn_evals;
  out.queries_loaded = c[AC_LOADED];
  out.queries_finished = c[AC_FINISHED];
  out.queries_rejected = c[AC_REJECTED];
  out.errors = s.errors;
  out.nn_precision = s.nn_precision;
  out.nn_audits = s.nn_audits;
  out.nn_audit_switches = s.nn_audit_switches;
  out.nn_audit_max_diff = s.nn_audit_max_diff;
}

int SelfplayEngine::drain(int maxRows, uint8_t* bin, float* glob, int16_t* pol, float* gt, int8_t* val,
                          int32_t* meta) {
  sync();
  unsigned long long cnt = 0;
  KC_HIP(hipMemcpy(&cnt, hd_.rCount, 8, hipMemcpyDeviceToHost));
  const int n = (int)std::min<unsigned long long>(cnt, (unsigned long long)std::max(maxRows, 0));
  const int A = hd_.A, P = hd_.P, pb = (A + 7) / 8;
  auto cp = [&](void* dst, const void* src, size_t rowBytes) {
    if(dst && n > 0)
      KC_HIP(hipMemcpy(dst, src, rowBytes * n, hipMemcpyDeviceToHost));
  };
  cp(bin, hd_.rBin, (size_t)NUM_SPATIAL * pb);
  cp(glob, hd_.rGlob, 4);
  cp(pol, hd_.rPol, (size_t)2 * P * 2);
  cp(gt, hd_.rGt, 64 * 4);
  cp(val, hd_.rVal, (size_t)5 * A);
  cp(meta, hd_.rMeta, 16);
  if(n > 0 && (unsigned long long)n < cnt) {
    // keep the undrained tail at the front of the buffer, in chunks of n rows so
    // no copy's source overlaps its destination
    const size_t rest = cnt - n;
    auto mv = [&](void* base, size_t rowBytes) {
      for(size_t off = 0; off < rest; off += (size_t)n) {
        const size_t k = std::min(rest - off, (size_t)n);
        KC_HIP(hipMemcpy((char*)base + rowBytes * off, (char*)base + rowBytes * (n + off), rowBytes * k,
                         hipMemcpyDeviceToDevice));
      }
    };
    mv(hd_.rBin, (size_t)NUM_SPATIAL * pb);
    mv(hd_.rGlob, 4);
    mv(hd_.rPol, (size_t)2 * P * 2);
    mv(hd_.rGt, 256);
    mv(hd_.rVal, (size_t)5 * A);
    mv(hd_.rMeta, 16);
  }
  unsigned long long left = cnt - (unsigned long long)n;
  KC_HIP(hipMemcpy(hd_.rCount, &left, 8, hipMemcpyHostToDevice));
  rowsDrained_ += n;
  return n;
}

void SelfplayEngine::stageRows(uint8_t* dst, int maxRows, unsigned long long* countOut, bool discardGames) {
  if(maxRows < hd_.rowCap)
    throw std::invalid_argument("stage_rows: the destination must hold the row capacity (" +
                                std::to_string(hd_.rowCap) + " rows)");
  launchStageRows(hd_, dd_, dst, countOut, discardGames, stream_);
  // kernel timings whose events completed are folded in without waiting (a run that
  // never drains synchronously would otherwise keep every event pending)
  size_t keep = 0;
  for(size_t i = 0; i < pending_.size(); i++) {
    const PendingTiming& p = pending_[i];
    if(hipEventQuery(p.b) == hipSuccess) {
      float ms = 0.0f;
      KC_HIP(hipEventElapsedTime(&ms, p.a, p.b));
      kernelMs_[p.which] += ms;
      kernelLaunches_[p.which]++;
      evPool_.push_back(p.a);
      evPool_.push_back(p.b);
    } else {
      pending_[keep++] = p;
    }
  }
  pending_.resize(keep);
}

int SelfplayEngine::drainGames(int maxGames, int32_t* header, uint8_t* moves) {
  sync();
  unsigned long long cnt = 0;
  KC_HIP(hipMemcpy(&cnt, hd_.gCount, 8, hipMemcpyDeviceToHost));
  const int n = (int)std::min<unsigned long long>(cnt, (unsigned long long)std::max(maxGames, 0));
  if(n > 0) {
    std::vector<GameRec> recs(n);
    KC_HIP(hipMemcpy(recs.data(), hd_.gRec, sizeof(GameRec) * n, hipMemcpyDeviceToHost));
    const int A = hd_.A, hw = hd_.matchMode ? 5 : 4;
    for(int i = 0; i < n; i++) {
      const GameRec& r = recs[i];
      if(header) {
        header[hw * i + 0] = r.slot;
        header[hw * i + 1] = r.gameNum;
        header[hw * i + 2] = r.numMoves;
        header[hw * i + 3] = r.winner;
        if(hd_.matchMode)
          header[hw * i + 4] = r.candidate;
      }
      if(moves)
        for(int t = 0; t < A; t++) {
          moves[((size_t)i * A + t) * 2 + 0] = t < r.numMoves ? r.cell[t] : 0xFF;
          moves[((size_t)i * A + t) * 2 + 1] = t < r.numMoves ? r.dir[t] : 0xFF;
        }
    }
    const size_t rest = cnt - n;
    for(size_t off = 0; off < rest; off += (size_t)n) {
      const size_t k = std::min(rest - off, (size_t)n);
      KC_HIP(hipMemcpy(hd_.gRec + off, hd_.gRec + n + off, sizeof(GameRec) * k, hipMemcpyDeviceToDevice));
    }
  }
  unsigned long long left = cnt - (unsigned long long)n;
  KC_HIP(hipMemcpy(hd_.gCount, &left, 8, hipMemcpyHostToDevice));
  return n;
}

// Rows per network launch: the configured cap, else the network's own (one wave of
// fused workgroups, split between the engines sharing the device; the layered path is
// uncapped), never more than the games.
int SelfplayEngine::nnCapFor(int G) const {
  if(userCap_ > 0)
    return userCap_;
  // (match play: the smaller of the two nets' own caps, on both nets' rows together)
  int cap = G;
  for(int n = 0; n < numNets_; n++) {
    const std::unique_ptr<NNEngine>& nn = nets_[n].nn;
    if(!nn)
      cap = std::min(cap, cus_ * NN_BOARDS_PER_WG);
    else if(nn->fused())
      cap = std::min(cap, nn->batchCap(cus_, enginesPerDevice_));
  }
  return cap;
}

void SelfplayEngine::setModel(const char* path) {
  if(!nets_[0].nn || hd_.matchMode)
    throw std::invalid_argument("engine runs the stand-in network (use_fake_net)");
  switchModel(loadModel(path));  // throws on a bad file; the current network stays
}

void SelfplayEngine::setModelBytes(const void* data, size_t bytes) {
  if(!nets_[0].nn || hd_.matchMode)
    throw std::invalid_argument("engine runs the stand-in network (use_fake_net)");
  switchModel(loadModelBytes(data, bytes, "<model bytes>"));
}

void SelfplayEngine::switchModel(const ModelHost& m) {
  std::unique_ptr<NNEngine> next(new NNEngine(m, xLen_, yLen_, winLen_, nnPath_));
  std::unique_ptr<ModelHost> keep(new ModelHost(m));
  sync();
  nets_[0].nn = std::move(next);
  nets_[0].model = std::move(keep);
  // the audit starts over for the new model
  nets_[0].auditSeen = 0.0f;
  KC_HIP(hipMemset(nets_[0].auditMax, 0, 4));
  // a reload may change the network path (fused <-> layered) and with it the default cap
  const int cap = nnCapFor(rows());
  if(cap != hd_.nnCap) {
    hd_.nnCap = cap;
    KC_HIP(hipMemcpy(&dd_->nnCap, &cap, sizeof(int), hipMemcpyHostToDevice));
  }
  // network generation: rows of games that span the switch carry it in [49] / [50]
  // (ChangedNeuralNet, play.cpp:1210-1226; trainingwrite.cpp:459-461)
  modelGen_++;
  KC_HIP(hipMemcpy(hd_.modelGen, &modelGen_, sizeof(int32_t), hipMemcpyHostToDevice));
  // cached evaluations belong to the previous network (the reference builds a new
  // NNEvaluator, and with it a new cache, per model: cpp/command/selfplay.cpp:150-200)
  if(hd_.cacheOn)
    KC_HIP(hipMemsetAsync(hd_.cKey, 0, sizeof(uint64_t) * 2 * ((size_t)hd_.cacheMask + 1), stream_));
}

void SelfplayEngine::gameInfo(int slot, int64_t* info) {
  if(slot < 0 || slot >= hd_.G)
    throw std::invalid_argument("slot out of range");
  sync();
  GameDev g;
  KC_HIP(hipMemcpy(&g, hd_.games + slot, sizeof(GameDev), hipMemcpyDeviceToHost));
  int64_t v[16] = {g.phase, g.rootK, g.liveCount, g.rootIdx, g.gameNum, g.root.turn, g.root.pla,
                   g.root.finished, g.root.winner, (int64_t)g.playouts, (int64_t)g.nnEvals, (int64_t)g.moves,
                   (int64_t)g.gamesFinished, g.root.lastCell, g.root.lastDir, (int64_t)g.rngCtr};
  memcpy(info, v, sizeof(v));
}

int SelfplayEngine::gameTree(int slot, int maxNodes, uint32_t* nodes, uint32_t* edges) {
  if(slot < 0 || slot >= hd_.G || maxNodes <= 0)
    throw std::invalid_argument("slot/max_nodes out of range");
  sync();
  std::vector<void*> tmp;
  // zeroed on the engine stream: a null-stream hipMemset is not ordered before work
  // on the non-blocking engine stream
  uint32_t* dn = devAlloc<uint32_t>(tmp, (size_t)maxNodes * 24, false);
  uint32_t* de = devAlloc<uint32_t>(tmp, (size_t)maxNodes * hd_.P * 3, false);
  int32_t* dc = devAlloc<int32_t>(tmp, 1, false);
  KC_HIP(hipMemsetAsync(dn, 0, (size_t)maxNodes * 24 * 4, stream_));
  KC_HIP(hipMemsetAsync(de, 0, (size_t)maxNodes * hd_.P * 3 * 4, stream_));
  KC_HIP(hipMemsetAsync(dc, 0, 4, stream_));
  launchGameTree(dd_, slot, maxNodes, dn, de, dc, stream_);
  KC_HIP(hipStreamSynchronize(stream_));
  int n = 0;
  KC_HIP(hipMemcpy(&n, dc, 4, hipMemcpyDeviceToHost));
  if(nodes)
    KC_HIP(hipMemcpy(nodes, dn, (size_t)maxNodes * 24 * 4, hipMemcpyDeviceToHost));
  if(edges)
    KC_HIP(hipMemcpy(edges, de, (size_t)maxNodes * hd_.P * 3 * 4, hipMemcpyDeviceToHost));
  for(void* p : tmp)
    (void)hipFree(p);
  return n;
}

int SelfplayEngine::gameTreePriors(int slot, int maxNodes, float* priors, float* nextPrior, int32_t* nextPos) {
  if(slot < 0 || slot >= hd_.G || maxNodes <= 0)
    throw std::invalid_argument("slot/max_nodes out of range");
  // (weak in search.h: a host-only link of the engine has no kernels; never null in the library)
  if(!launchGameTreePriors)
    throw InternalError("game_tree_priors: this build has no export kernel");
  sync();
  std::vector<void*> tmp;
  struct Guard {
    std::vector<void*>& t;
    ~Guard() {
      for(void* p : t)
        (void)hipFree(p);
    }
  } guard{tmp};
  const size_t np = (size_t)maxNodes * hd_.P;
  uint32_t* dp = devAlloc<uint32_t>(tmp, np, false);
  uint32_t* dn = devAlloc<uint32_t>(tmp, (size_t)maxNodes * 2, false);
  int32_t* dorder = devAlloc<int32_t>(tmp, (size_t)maxNodes, false);
  int32_t* dc = devAlloc<int32_t>(tmp, 1, false);
  KC_HIP(hipMemsetAsync(dp, 0, np * 4, stream_));
  KC_HIP(hipMemsetAsync(dn, 0, (size_t)maxNodes * 2 * 4, stream_));
  KC_HIP(hipMemsetAsync(dc, 0, 4, stream_));
  launchGameTreePriors(dd_, slot, maxNodes, dp, dn, dorder, dc, stream_);
  KC_HIP(hipStreamSynchronize(stream_));
  int n = 0;
  KC_HIP(hipMemcpy(&n, dc, 4, hipMemcpyDeviceToHost));
  if(priors)
    KC_HIP(hipMemcpy(priors, dp, np * 4, hipMemcpyDeviceToHost));
  if(nextPrior || nextPos) {
    std::vector<uint32_t> nx((size_t)maxNodes * 2);
    KC_HIP(hipMemcpy(nx.data(), dn, nx.size() * 4, hipMemcpyDeviceToHost));
    for(int i = 0; i < maxNodes; i++) {
      if(nextPrior)
        memcpy(&nextPrior[i], &nx[2 * (size_t)i], 4);
      if(nextPos)
        nextPos[i] = (int32_t)nx[2 * (size_t)i + 1];
    }
  }
  return n;
}

void SelfplayEngine::rootPolicy(int slot, float* out) {
  if(slot < 0 || slot >= hd_.G)
    throw std::invalid_argument("slot out of range");
  sync();
  KC_HIP(hipMemcpy(out, hd_.rootNoised + (size_t)slot * hd_.P, sizeof(float) * hd_.P, hipMemcpyDeviceToHost));
}

uint64_t SelfplayEngine::timedNNEvals() {
  sync();
  unsigned long long v = 0;
  KC_HIP(hipMemcpy(&v, hd_.nnTimedEvals, 8, hipMemcpyDeviceToHost));
  return v;
}

void SelfplayEngine::kernelTime(int which, double& ms, uint64_t& launches) {
  resolveTiming();
  if(which < 0 || which > 4)
    throw std::invalid_argument("which must be 0..4");
  ms = kernelMs_[which];
  launches = kernelLaunches_[which];
}

}  // namespace kc
