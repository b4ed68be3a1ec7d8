// C ABI (include/katacoffee.h): argument checking, error capture, dispatch.
// No C++ exception crosses this boundary; failures return COFFEE_E* with the
// message in coffee_last_error().
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>

#include "../../include/katacoffee.h"
#include "engine.h"
#include "model.h"
#include "npzwrite.h"
#include "selfplay.h"

namespace kc {

// ---- per-geometry table cache ----
namespace {
std::mutex gTablesMu;
std::map<std::tuple<int, int, int, int>, std::pair<DTables*, DTables*>> gTables;  // (dev,X,Y,W) -> host, device
}  // namespace

static std::pair<DTables*, DTables*> tablesFor(int X, int Y, int W) {
  int dev = 0;
  KC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(gTablesMu);
  auto key = std::make_tuple(dev, X, Y, W);
  auto it = gTables.find(key);
  if(it != gTables.end())
    return it->second;
  DTables* h = new DTables(buildTables(X, Y, W));
  DTables* d = nullptr;
  KC_HIP(hipMalloc(&d, sizeof(DTables)));
  KC_HIP(hipMemcpy(d, h, sizeof(DTables), hipMemcpyHostToDevice));
  gTables[key] = {h, d};
  return {h, d};
}

const DTables* deviceTables(int X, int Y, int W) { return tablesFor(X, Y, W).second; }
const DTables& hostTables(int X, int Y, int W) { return *tablesFor(X, Y, W).first; }

}  // namespace kc

using namespace kc;

static thread_local std::string gLastError;

template <class F>
static int guarded(F&& f) {
  try {
    gLastError.clear();
    f();
    return COFFEE_OK;
  } catch(const HipError& e) {
    gLastError = e.what();
    return COFFEE_EHIP;
  } catch(const std::invalid_argument& e) {
    gLastError = e.what();
    return COFFEE_EINVAL;
  } catch(const InternalError& e) {
    gLastError = e.what();
    return COFFEE_EINTERNAL;
  } catch(const std::runtime_error& e) {
    gLastError = e.what();
    return COFFEE_EIO;
  } catch(const std::exception& e) {
    gLastError = e.what();
    return COFFEE_EINTERNAL;
  } catch(...) {
    gLastError = "unknown error";
    return COFFEE_EINTERNAL;
  }
}

static void need(bool ok, const char* what) {
  if(!ok)
    throw std::invalid_argument(what);
}

static void checkGeom(int x, int y, int w) {
  need(x >= 2 && y >= 2 && x <= MAX_LEN && y <= MAX_LEN, "board size must be 2..10 x 2..10");
  need(w >= 2 && w <= (x > y ? x : y), "win_len must be in 2..max(x, y)");
}

extern "C" {

const char* coffee_last_error(void) { return gLastError.c_str(); }
int coffee_abi_version(void) { return 108; }

int coffee_device_count(int* count) {
  return guarded([&] {
    need(count != nullptr, "count is NULL");
    KC_HIP(hipGetDeviceCount(count));
  });
}
int coffee_set_device(int device) {
  return guarded([&] { KC_HIP(hipSetDevice(device)); });
}
int coffee_device_compute_units(int device, int* cus) {
  return guarded([&] {
    need(cus != nullptr, "cus is NULL");
    KC_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
  });
}
int coffee_malloc(void** p, uint64_t bytes) {
  return guarded([&] {
    need(p != nullptr, "pointer is NULL");
    KC_HIP(hipMalloc(p, bytes ? bytes : 1));
  });
}
int coffee_free(void* p) {
  return guarded([&] { KC_HIP(hipFree(p)); });
}
int coffee_memcpy(void* dst, const void* src, uint64_t bytes, int kind) {
  return guarded([&] {
    need(kind >= 0 && kind <= 2, "kind must be 0, 1 or 2");
    hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    KC_HIP(hipMemcpy(dst, src, bytes, k));
  });
}
int coffee_synchronize(void) {
  return guarded([&] { KC_HIP(hipDeviceSynchronize()); });
}

int coffee_rules_batch(int x, int y, int win_len, int n, const uint8_t* cells, const int8_t* last_cell,
                       const int8_t* last_dir, const uint8_t* pla, uint8_t* legal, uint8_t* has_legal, void* stream) {
  return guarded([&] {
    checkGeom(x, y, win_len);
    need(n >= 0, "n must be >= 0");
    need(n == 0 || (cells && last_cell && last_dir && pla && legal && has_legal), "NULL buffer");
    launchRulesBatch(deviceTables(x, y, win_len), n, cells, last_cell, last_dir, pla, legal, has_legal,
                     (hipStream_t)stream);
  });
}

int coffee_play_batch(int x, int y, int win_len, int n, const uint8_t* cells, const int8_t* last_cell,
                      const int8_t* last_dir, const uint8_t* pla, const int32_t* move, uint8_t* out_cells,
                      uint8_t* finished, uint8_t* winner, int32_t* max_run, uint64_t* pos_hash,
                      uint64_t* state_hash, void* stream) {
  return guarded([&] {
    checkGeom(x, y, win_len);
    need(n >= 0, "n must be >= 0");
    need(n == 0 || (cells && last_cell && last_dir && pla && move && out_cells && finished && winner && max_run &&
                    pos_hash && state_hash),
         "NULL buffer");
    launchPlayBatch(deviceTables(x, y, win_len), n, cells, last_cell, last_dir, pla, move, out_cells, finished,
                    winner, max_run, pos_hash, state_hash, (hipStream_t)stream);
  });
}

int coffee_encode_batch(int x, int y, int win_len, int n, const uint8_t* cells, const int8_t* hist_cell,
                        const int8_t* hist_dir, const uint8_t* pla, const int32_t* sym, uint64_t* packed,
                        float* planes, void* stream) {
  return guarded([&] {
    checkGeom(x, y, win_len);
    need(n >= 0, "n must be >= 0");
    need(n == 0 || (cells && hist_cell && hist_dir && pla && sym && packed), "NULL buffer");
    launchEncodeBatch(deviceTables(x, y, win_len), n, cells, hist_cell, hist_dir, pla, sym, packed, planes,
                      (hipStream_t)stream);
  });
}

int coffee_model_write_random(const char* arch, uint64_t seed, const char* path) {
  return guarded([&] {
    need(arch && path, "NULL argument");
    saveModel(path, randomModel(modelCfgByName(arch), seed));
  });
}

int coffee_model_flops(const char* path, int area, double* flops) {
  return guarded([&] {
    need(path && flops && area > 0, "bad argument");
    ModelHost m = loadModel(path);
    *flops = modelFlopsPerEval(m.cfg, area);
  });
}

struct coffee_nn {
  NNEngine* eng;
  int x, y, w;
};

int coffee_nn_create(const char* model_path, int x, int y, int win_len, coffee_nn** out) {
  return coffee_nn_create2(model_path, x, y, win_len, COFFEE_NN_DEFAULT, out);
}

int coffee_nn_create2(const char* model_path, int x, int y, int win_len, int precision, coffee_nn** out) {
  return guarded([&] {
    need(model_path && out, "NULL argument");
    need(precision >= COFFEE_NN_DEFAULT && precision <= COFFEE_NN_FAST, "unknown precision");
    checkGeom(x, y, win_len);
    ModelHost m = loadModel(model_path);
    (void)deviceTables(x, y, win_len);
    coffee_nn* h = new coffee_nn{nullptr, x, y, win_len};
    try {
      h->eng = new NNEngine(m, x, y, win_len, precision);
    } catch(...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int coffee_nn_forward(coffee_nn* h, int n, const uint64_t* in, float* out, void* stream) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    need(n >= 0, "n must be >= 0");
    need(n == 0 || (in && out), "NULL buffer");
    h->eng->forward(n, in, out, (hipStream_t)stream);
  });
}

int coffee_nn_forward2(coffee_nn* h, int n, const uint64_t* in, const int32_t* sym, float* out, void* stream) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    need(n >= 0, "n must be >= 0");
    need(n == 0 || (in && sym && out), "NULL buffer");
    h->eng->forward(n, in, out, (hipStream_t)stream);
    launchCanonicalRows(deviceTables(h->x, h->y, h->w), n, sym, out, (hipStream_t)stream);
  });
}

int coffee_nn_is_fused(coffee_nn* h, int* fused) {
  return guarded([&] {
    need(h && h->eng && fused, "NULL argument");
    *fused = h->eng->fused() ? 1 : 0;
  });
}

int coffee_nn_precision(coffee_nn* h, int* precision, float* calib_err) {
  return guarded([&] {
    need(h && h->eng && precision, "NULL argument");
    *precision = h->eng->precision();
    if(calib_err)
      *calib_err = h->eng->calibrationError();
  });
}

int coffee_nn_destroy(coffee_nn* h) {
  return guarded([&] {
    if(h) {
      delete h->eng;
      delete h;
    }
  });
}

int coffee_fake_net(int x, int y, int win_len, int n, const uint64_t* in, float* out, void* stream) {
  return guarded([&] {
    checkGeom(x, y, win_len);
    need(n >= 0, "n must be >= 0");
    need(n == 0 || (in && out), "NULL buffer");
    launchFakeNet(deviceTables(x, y, win_len), n, in, out, (hipStream_t)stream);
  });
}

void coffee_search_params_default(coffee_search_params* p) {
  if(!p)
    return;
  // cpp/configs/training/selfplay1.cfg (SURVEY §8d benchmark settings)
  p->max_visits = 600;
  p->cpuct_exploration = 1.1f;
  p->cpuct_exploration_log = 0.0f;
  p->cpuct_exploration_base = 500.0f;
  p->fpu_reduction_max = 0.2f;
  p->root_fpu_reduction_max = 0.0f;
  p->fpu_loss_prop = 0.0f;
  p->root_fpu_loss_prop = 0.0f;
  p->fpu_parent_weight_by_visited_policy = 1;
  p->fpu_parent_weight_by_visited_policy_pow = 2.0f;
  p->value_weight_exponent = 0.5f;
  p->root_noise_enabled = 1;
  p->root_dirichlet_noise_total_concentration = 10.83f;
  p->root_dirichlet_noise_weight = 0.25f;
  p->root_policy_temperature = 1.1f;
  p->root_policy_temperature_early = 1.25f;
  p->root_desired_per_child_visits_coeff = 2.0f;
  p->root_num_symmetries_to_sample = 4;
  p->chosen_move_temperature = 0.15f;
  p->chosen_move_temperature_early = 0.75f;
  p->chosen_move_temperature_halflife = 19.0f;
  p->chosen_move_subtract = 0.0f;
  p->chosen_move_prune = 1.0f;
  p->use_lcb_for_selection = 1;
  p->lcb_stdevs = 5.0f;
  p->min_visit_prop_for_lcb = 0.15f;
  p->subtree_value_bias_factor = 0.30f;
  p->subtree_value_bias_weight_exponent = 0.8f;
  p->subtree_value_bias_free_prop = 0.8f;
  p->use_graph_search = 1;
  // play settings: benchmark mode (one row per move at full visits)
  p->cheap_search_prob = 0.0f;
  p->cheap_search_visits = 100;
  p->cheap_search_target_weight = 0.0f;
  p->reduce_visits = 0;
  p->reduce_visits_threshold = 0.9f;
  p->reduce_visits_threshold_lookback = 3;
  p->reduced_visits_min = 100;
  p->reduced_visits_weight = 0.1f;
  p->policy_surprise_data_weight = 0.0f;
  p->value_surprise_data_weight = 0.0f;
  p->init_games_with_policy = 0;
  p->policy_init_area_prop = 0.04f;
  p->policy_init_area_temperature = 1.0f;
  p->early_fork_game_prob = 0.0f;
  p->early_fork_game_expected_move_prop = 0.025f;
  p->fork_game_prob = 0.0f;
  p->fork_game_min_choices = 3;
  p->early_fork_game_max_choices = 12;
  p->fork_game_max_choices = 36;
  p->side_position_prob = 0.0f;
  p->record_tree_positions = 0;
  p->record_tree_threshold = 0;
  p->record_tree_target_weight = 0.0f;
}

struct coffee_selfplay {
  SelfplayEngine* eng;
};

int coffee_selfplay_create(const coffee_selfplay_config* cfg, coffee_selfplay** out) {
  return guarded([&] {
    need(cfg && out, "NULL argument");
    checkGeom(cfg->x, cfg->y, cfg->win_len);
    coffee_selfplay* h = new coffee_selfplay{nullptr};
    try {
      h->eng = new SelfplayEngine(*cfg);
    } catch(...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int coffee_selfplay_step(coffee_selfplay* h, int rounds, void* stream) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    need(rounds >= 0, "rounds must be >= 0");
    h->eng->step(rounds, (hipStream_t)stream);
  });
}

int coffee_selfplay_sync(coffee_selfplay* h) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    h->eng->sync();
  });
}

int coffee_selfplay_stats_get(coffee_selfplay* h, coffee_selfplay_stats* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->stats(*out);
  });
}

int coffee_selfplay_drain_rows(coffee_selfplay* h, int max_rows, uint8_t* bin, float* glob, int16_t* pol,
                               float* gtgt, int8_t* value, int32_t* meta, int* n_out) {
  return guarded([&] {
    need(h && h->eng && n_out, "NULL argument");
    *n_out = h->eng->drain(max_rows, bin, glob, pol, gtgt, value, meta);
  });
}

int coffee_row_bytes(int x, int y, int* bytes) {
  return guarded([&] {
    need(bytes != nullptr, "NULL argument");
    need(x >= 2 && y >= 2 && x <= MAX_LEN && y <= MAX_LEN, "bad shape");
    *bytes = rowBytes(x * y);
  });
}

int coffee_selfplay_row_capacity(coffee_selfplay* h, int* rows) {
  return guarded([&] {
    need(h && h->eng && rows, "NULL argument");
    *rows = h->eng->dev().rowCap;
  });
}

int coffee_selfplay_stream(coffee_selfplay* h, void** stream) {
  return guarded([&] {
    need(h && h->eng && stream, "NULL argument");
    *stream = (void*)h->eng->stream();
  });
}

int coffee_selfplay_stage_rows(coffee_selfplay* h, void* dst, int max_rows, uint64_t* count, int flags) {
  return guarded([&] {
    need(h && h->eng && dst && count, "NULL argument");
    need((flags & ~COFFEE_STAGE_DISCARD_GAMES) == 0, "unknown flags");
    h->eng->stageRows((uint8_t*)dst, max_rows, (unsigned long long*)count, (flags & COFFEE_STAGE_DISCARD_GAMES) != 0);
  });
}

int coffee_selfplay_drain_games(coffee_selfplay* h, int max_games, int32_t* header, uint8_t* moves, int* n_out) {
  return guarded([&] {
    need(h && h->eng && n_out, "NULL argument");
    need(max_games >= 0, "max_games must be >= 0");
    *n_out = h->eng->drainGames(max_games, header, moves);
  });
}

int coffee_selfplay_set_model(coffee_selfplay* h, const char* model_path) {
  return guarded([&] {
    need(h && h->eng && model_path, "NULL argument");
    h->eng->setModel(model_path);
  });
}

int coffee_selfplay_set_model_bytes(coffee_selfplay* h, const void* data, uint64_t bytes) {
  return guarded([&] {
    need(h && h->eng && data, "NULL argument");
    h->eng->setModelBytes(data, (size_t)bytes);
  });
}

int coffee_selfplay_destroy(coffee_selfplay* h) {
  return guarded([&] {
    if(h) {
      delete h->eng;
      delete h;
    }
  });
}

// ---- two-network match play: the self-play engine in match mode ----

void coffee_match_params_default(coffee_search_params* p) {
  if(!p)
    return;
  coffee_search_params_default(p);  // play settings all off
  // cpp/configs/training/gatekeeper1.cfg:49, :72-80, :95-106
  p->max_visits = 150;
  p->chosen_move_temperature_early = 0.5f;
  p->chosen_move_temperature_halflife = 19.0f;
  p->chosen_move_temperature = 0.2f;
  p->chosen_move_subtract = 0.0f;
  p->chosen_move_prune = 1.0f;
  p->use_lcb_for_selection = 1;
  p->lcb_stdevs = 5.0f;
  p->min_visit_prop_for_lcb = 0.15f;
  p->cpuct_exploration = 1.1f;
  p->cpuct_exploration_log = 0.0f;
  p->fpu_reduction_max = 0.2f;
  p->root_fpu_reduction_max = 0.1f;
  p->value_weight_exponent = 0.5f;
  p->subtree_value_bias_factor = 0.35f;
  p->subtree_value_bias_weight_exponent = 0.8f;
  p->use_graph_search = 1;
  // not in that config: the reference's defaults (searchparams.cpp), root noise off
  p->root_noise_enabled = 0;
  p->root_policy_temperature = 1.0f;
  p->root_policy_temperature_early = 1.0f;
  p->root_desired_per_child_visits_coeff = 0.0f;
  p->root_num_symmetries_to_sample = 1;
}

struct coffee_match {
  SelfplayEngine* eng;
};

int coffee_match_create2(const coffee_match_config* cfg, const coffee_match_options* opts, coffee_match** out) {
  return guarded([&] {
    need(cfg && out, "NULL argument");
    coffee_match* h = new coffee_match{nullptr};
    try {
      h->eng = new SelfplayEngine(*cfg, opts);  // validates config and options before its first HIP call
    } catch(...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int coffee_match_create(const coffee_match_config* cfg, coffee_match** out) {
  return coffee_match_create2(cfg, nullptr, out);
}

int coffee_match_elo(int64_t wins, int64_t draws, int64_t losses, double* score, double* elo, double* elo_lo,
                     double* elo_hi, double* los) {
  return guarded([&] {
    need(wins >= 0 && draws >= 0 && losses >= 0, "wins, draws and losses must be >= 0");
    need(wins + draws + losses > 0, "no games: wins + draws + losses must be > 0");
    const double W = (double)wins, D = (double)draws, L = (double)losses, N = W + D + L;
    const double p = (W + D / 2.0) / N;
    const double var = (W * (1.0 - p) * (1.0 - p) + D * (0.5 - p) * (0.5 - p) + L * p * p) / N;
    const double se = std::sqrt(var / N);
    auto eloOf = [](double x) {
      if(x <= 0.0)
        return -HUGE_VAL;
      if(x >= 1.0)
        return HUGE_VAL;
      return -400.0 * std::log10(1.0 / x - 1.0);
    };
    if(score)
      *score = p;
    if(elo)
      *elo = eloOf(p);
    if(elo_lo)
      *elo_lo = eloOf(p - 1.96 * se);
    if(elo_hi)
      *elo_hi = eloOf(p + 1.96 * se);
    if(los)
      *los = W + L > 0.0 ? 0.5 * std::erfc(-(W - L) / std::sqrt(2.0 * (W + L))) : 0.5;
  });
}

int coffee_match_step(coffee_match* h, int rounds, void* stream) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    need(rounds >= 0, "rounds must be >= 0");
    h->eng->step(rounds, (hipStream_t)stream);
  });
}

int coffee_match_sync(coffee_match* h) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    h->eng->sync();
  });
}

int coffee_match_stream(coffee_match* h, void** stream) {
  return guarded([&] {
    need(h && h->eng && stream, "NULL argument");
    *stream = (void*)h->eng->stream();
  });
}

int coffee_match_destroy(coffee_match* h) {
  return guarded([&] {
    if(h) {
      delete h->eng;
      delete h;
    }
  });
}

int coffee_match_stats_get(coffee_match* h, coffee_match_stats* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->matchStats(*out);
  });
}

int coffee_match_drain_games(coffee_match* h, int max_games, int32_t* header, uint8_t* moves, int* n_out) {
  return guarded([&] {
    need(h && h->eng && n_out, "NULL argument");
    need(max_games >= 0, "max_games must be >= 0");
    *n_out = h->eng->drainGames(max_games, header, moves);
  });
}

int coffee_match_score(const int32_t* header, int n, double* candidate_points, double* baseline_points) {
  return guarded([&] {
    need(n >= 0 && (n == 0 || header) && candidate_points && baseline_points, "bad argument");
    double c = 0.0, b = 0.0;
    for(int i = 0; i < n; i++) {
      const int winner = header[5 * i + 3], cand = header[5 * i + 4];
      need((cand == 1 || cand == 2) && winner >= 0 && winner <= 2, "header: winner 0..2 and candidate colour 1 or 2");
      if(winner == 0) {
        c += 0.5;
        b += 0.5;
      } else if(winner == cand) {
        c += 1.0;
      } else {
        b += 1.0;
      }
    }
    *candidate_points = c;
    *baseline_points = b;
  });
}

int coffee_match_game_info(coffee_match* h, int slot, int64_t* info) {
  return guarded([&] {
    need(h && h->eng && info, "NULL argument");
    h->eng->gameInfo(slot, info);
  });
}

int coffee_match_game_tree(coffee_match* h, int slot, int max_nodes, uint32_t* nodes, uint32_t* edges,
                           int* n_nodes) {
  return guarded([&] {
    need(h && h->eng && n_nodes, "NULL argument");
    *n_nodes = h->eng->gameTree(slot, max_nodes, nodes, edges);
  });
}

int coffee_match_root_policy(coffee_match* h, int slot, float* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->rootPolicy(slot, out);
  });
}

// ---- batched position analysis: the self-play engine in analysis mode ----

void coffee_analysis_params_default(coffee_search_params* p) {
  if(!p)
    return;
  coffee_match_params_default(p);
  // cpp/configs/analysis_example.cfg:66, :278-285 (the commented values are the defaults)
  p->max_visits = 500;
  p->use_lcb_for_selection = 1;
  p->lcb_stdevs = 5.0f;
  p->min_visit_prop_for_lcb = 0.15f;
  p->root_num_symmetries_to_sample = 1;
  p->root_noise_enabled = 0;
  // the reported play-selection values are unpruned
  p->chosen_move_subtract = 0.0f;
  p->chosen_move_prune = 0.0f;
}

struct coffee_analysis {
  SelfplayEngine* eng;
};

int coffee_analysis_create(const coffee_analysis_config* cfg, coffee_analysis** out) {
  return guarded([&] {
    need(cfg && out, "NULL argument");
    coffee_analysis* h = new coffee_analysis{nullptr};
    try {
      h->eng = new SelfplayEngine(*cfg);  // validates the config before its first HIP call
    } catch(...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int coffee_analysis_step(coffee_analysis* h, int rounds, void* stream) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    need(rounds >= 0, "rounds must be >= 0");
    h->eng->step(rounds, (hipStream_t)stream);
  });
}

int coffee_analysis_sync(coffee_analysis* h) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    h->eng->sync();
  });
}

int coffee_analysis_stream(coffee_analysis* h, void** stream) {
  return guarded([&] {
    need(h && h->eng && stream, "NULL argument");
    *stream = (void*)h->eng->stream();
  });
}

int coffee_analysis_destroy(coffee_analysis* h) {
  return guarded([&] {
    if(h) {
      delete h->eng;
      delete h;
    }
  });
}

int coffee_analysis_query_check(int x, int y, int win_len, const coffee_analysis_query* q) {
  return guarded([&] {
    need(q != nullptr, "NULL argument");
    checkGeom(x, y, win_len);
    validateAnalysisQuery(x, y, *q);
  });
}

int coffee_analysis_submit(coffee_analysis* h, const coffee_analysis_query* queries, int n, int* accepted) {
  return guarded([&] {
    need(h && h->eng && accepted, "NULL argument");
    need(n >= 0 && (n == 0 || queries), "n must be >= 0 and queries non-NULL");
    *accepted = 0;
    *accepted = h->eng->analysisSubmit(queries, nullptr, n);
  });
}

int coffee_analysis_drain(coffee_analysis* h, int max, coffee_analysis_result* header_out,
                          coffee_analysis_move* moves_out, int* n_out) {
  return guarded([&] {
    need(h && h->eng && n_out, "NULL argument");
    need(max >= 0, "max must be >= 0");
    *n_out = h->eng->analysisDrain(max, header_out, moves_out);
  });
}

int coffee_analysis_set_root_options(coffee_analysis* h, const coffee_analysis_root_options* opts) {
  return guarded([&] {
    need(h && h->eng && opts, "NULL argument");
    h->eng->setRootOptions(*opts);
  });
}

int coffee_analysis_submit2(coffee_analysis* h, const coffee_analysis_query* queries,
                            const coffee_analysis_restrict* restrict_in, int n, int* accepted) {
  return guarded([&] {
    need(h && h->eng && accepted, "NULL argument");
    need(n >= 0 && (n == 0 || queries), "n must be >= 0 and queries non-NULL");
    *accepted = 0;
    *accepted = h->eng->analysisSubmit(queries, restrict_in, n);
  });
}

int coffee_analysis_drain2(coffee_analysis* h, int max, coffee_analysis_result* header_out,
                           coffee_analysis_move* moves_out, coffee_analysis_root_info* root_out,
                           float* policy_out, int* n_out) {
  return guarded([&] {
    need(h && h->eng && n_out, "NULL argument");
    need(max >= 0, "max must be >= 0");
    *n_out = h->eng->analysisDrain(max, header_out, moves_out, root_out, policy_out);
  });
}

// The symmetry tables of a geometry without a device (coffee_root_mask / coffee_symmetry_move).
static const DTables& hostOnlyTables(int x, int y, int w) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, DTables*> cache;
  std::lock_guard<std::mutex> lk(mu);
  DTables*& t = cache[std::make_tuple(x, y, w)];
  if(!t)
    t = new DTables(buildTables(x, y, w));
  return *t;
}

int coffee_root_mask(int x, int y, int win_len, const uint8_t* colours, const int32_t* hist_cell,
                     const int32_t* hist_dir, int n_hist, const uint32_t* legal_bits, const uint32_t* avoid_bits,
                     int mode, int prune, uint32_t* mask_out, uint32_t* syms_out) {
  int left = 0;
  const int rc = guarded([&] {
    checkGeom(x, y, win_len);
    need(colours && legal_bits && mask_out && syms_out, "NULL argument");
    need(n_hist >= 0 && n_hist <= HIST && (n_hist == 0 || (hist_cell && hist_dir)), "n_hist must be in 0..5 with both arrays");
    need(prune == 0 || prune == 1, "prune must be 0 or 1");
    const DTables& T = hostOnlyTables(x, y, win_len);
    coffee_analysis_restrict r;
    memset(&r, 0, sizeof(r));
    r.mode = mode;
    if(mode != RM_NONE) {
      need(avoid_bits != nullptr, "avoid_bits is NULL");
      memcpy(r.avoid, avoid_bits, sizeof(r.avoid));
    }
    validateAnalysisRestrict(x, y, 0, r);
    const RootGeom g{T.X, T.Y, T.A, T.P, &T.symCell[0][0], &T.symDir[0][0]};
    RootPos p;
    memset(&p, 0, sizeof(p));
    for(int c = 0; c < T.A; c++) {
      need(colours[c] <= 2, "colours must be 0, 1 or 2");
      if(colours[c] != 0)
        p.stones[2 * (colours[c] - 1) + (c >> 6)] |= 1ULL << (c & 63);
    }
    for(int k = 0; k < HIST; k++) {
      p.histCell[k] = -1;
      p.histDir[k] = 4;
      if(k < n_hist && hist_cell[k] >= 0) {
        need(hist_cell[k] < T.A && hist_dir[k] >= 0 && hist_dir[k] <= 4, "history entry out of range");
        p.histCell[k] = hist_cell[k];
        p.histDir[k] = hist_dir[k];
      }
    }
    int masked = 0;
    left = rmRootMask(g, p, legal_bits, r.avoid, mode, prune != 0, mask_out, syms_out, &masked);
  });
  return rc != COFFEE_OK ? rc : left;
}

int coffee_symmetry_move(int x, int y, int sym, int move) {
  int image = 0;
  const int rc = guarded([&] {
    need(x >= 2 && y >= 2 && x <= MAX_LEN && y <= MAX_LEN, "board size must be 2..10 x 2..10");
    need(sym >= 0 && sym < 8, "sym must be in 0..7");
    need(move >= 0 && move < 4 * x * y, "move must be a policy position");
    const DTables& T = hostOnlyTables(x, y, 2);
    const RootGeom g{T.X, T.Y, T.A, T.P, &T.symCell[0][0], &T.symDir[0][0]};
    image = rmImage(g, sym, move);
  });
  return rc != COFFEE_OK ? rc : image;
}

int coffee_analysis_stats_get(coffee_analysis* h, coffee_analysis_stats* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->analysisStats(*out);
  });
}

int coffee_analysis_game_info(coffee_analysis* h, int slot, int64_t* info) {
  return guarded([&] {
    need(h && h->eng && info, "NULL argument");
    h->eng->gameInfo(slot, info);
  });
}

int coffee_analysis_game_tree(coffee_analysis* h, int slot, int max_nodes, uint32_t* nodes, uint32_t* edges,
                              int* n_nodes) {
  return guarded([&] {
    need(h && h->eng && n_nodes, "NULL argument");
    *n_nodes = h->eng->gameTree(slot, max_nodes, nodes, edges);
  });
}

int coffee_analysis_root_policy(coffee_analysis* h, int slot, float* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->rootPolicy(slot, out);
  });
}

int coffee_write_npz(const char* path, int n, int x, int y, const uint8_t* bin, const float* glob,
                     const int16_t* pol, const float* gtgt, const int8_t* value) {
  return guarded([&] {
    need(path != nullptr, "NULL path");
    need(n >= 0 && x >= 2 && y >= 2 && x <= MAX_LEN && y <= MAX_LEN, "bad shape");
    writeNpz(path, n, x, y, bin, glob, pol, gtgt, value);
  });
}

int coffee_selfplay_game_info(coffee_selfplay* h, int slot, int64_t* info) {
  return guarded([&] {
    need(h && h->eng && info, "NULL argument");
    h->eng->gameInfo(slot, info);
  });
}

int coffee_selfplay_game_tree(coffee_selfplay* h, int slot, int max_nodes, uint32_t* nodes, uint32_t* edges,
                              int* n_nodes) {
  return guarded([&] {
    need(h && h->eng && n_nodes, "NULL argument");
    *n_nodes = h->eng->gameTree(slot, max_nodes, nodes, edges);
  });
}

int coffee_selfplay_root_policy(coffee_selfplay* h, int slot, float* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->rootPolicy(slot, out);
  });
}

// ---- uncertainty weighting (uncertainty.h: the sequences the search kernels run) ----

void coffee_uncertainty_params_default(coffee_uncertainty_params* p) {
  if(!p)
    return;
  // searchparams.cpp:29-32 (off), gatekeeper1.cfg:108-110 / setup.cpp:539-562 values
  p->use_uncertainty = 0;
  p->uncertainty_coeff = 0.25f;
  p->uncertainty_exponent = 1.0f;
  p->uncertainty_max_weight = 8.0f;
}

int coffee_uncertainty_weight(const coffee_uncertainty_params* p, float st_error_logit, float* err, float* weight) {
  return guarded([&] {
    need(p != nullptr, "NULL argument");
    const Unc u = toUnc(*p);
    const float e = stErrorOf(st_error_logit);
    if(err)
      *err = e;
    if(weight)
      *weight = uncWeightOf(u, e);
  });
}

int coffee_selfplay_set_uncertainty(coffee_selfplay* h, const coffee_uncertainty_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setUncertainty(*p);
  });
}

int coffee_match_set_uncertainty(coffee_match* h, const coffee_uncertainty_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setUncertainty(*p);
  });
}

int coffee_analysis_set_uncertainty(coffee_analysis* h, const coffee_uncertainty_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setUncertainty(*p);
  });
}

// ---- variance-scaled exploration and noise pruning (explore.h: the sequences the kernels run) ----

void coffee_exploration_params_default(coffee_exploration_params* p) {
  if(!p)
    return;
  // searchparams.cpp (both off); the other fields as setup.cpp:453-470, :520-537 load them
  p->use_noise_pruning = 0;
  p->noise_prune_utility_scale = 0.15f;
  p->noise_pruning_cap = FLT_MAX;
  p->cpuct_utility_stdev_prior = 0.40f;
  p->cpuct_utility_stdev_prior_weight = 2.0f;
  p->cpuct_utility_stdev_scale = 0.0f;
}

int coffee_explore_stdev_factor(const coffee_exploration_params* p, int64_t visits, float weight_sum,
                                float utility_avg, float utility_sq_avg, float* factor) {
  return guarded([&] {
    need(p && factor, "NULL argument");
    const Expl e = toExpl(*p);
    const uint32_t v = visits <= 0 ? 0u : (visits > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)visits);
    *factor = exploreStdevFactor(e, v, weight_sum, utility_avg, utility_sq_avg);
  });
}

int coffee_prune_noise_weight(const coffee_exploration_params* p, int n, const float* weight, const float* utility,
                              const float* prior, float* new_weight, float* new_total) {
  return guarded([&] {
    need(p != nullptr && n >= 0, "NULL argument or n < 0");
    need(n == 0 || (weight && utility && prior), "NULL argument");
    const Expl e = toExpl(*p);
    float total = 0.0f;
    for(int i = 0; i < n; i++)
      total = total + weight[i];
    if(!pruneNoiseApplies(n, total)) {  // (the scan itself: use_noise_pruning is not consulted)
      if(new_weight)
        for(int i = 0; i < n; i++)
          new_weight[i] = weight[i];
      if(new_total)
        *new_total = total;
      return;
    }
    PruneScan sc{0.0f, 0.0f, 0.0f};
    for(int i = 0; i < n; i++) {
      const float nw = pruneNoiseStep(e, sc, weight[i], utility[i], prior[i]);
      if(new_weight)
        new_weight[i] = nw;
    }
    if(new_total)
      *new_total = sc.wSum;
  });
}

int coffee_selfplay_set_exploration(coffee_selfplay* h, const coffee_exploration_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setExploration(-1, *p);
  });
}

int coffee_analysis_set_exploration(coffee_analysis* h, const coffee_exploration_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setExploration(-1, *p);
  });
}

int coffee_match_set_exploration(coffee_match* h, int side, const coffee_exploration_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setExploration(side, *p);
  });
}

int coffee_selfplay_game_tree_priors(coffee_selfplay* h, int slot, int max_nodes, float* priors, float* next_prior,
                                     int32_t* next_pos, int* n_nodes) {
  return guarded([&] {
    need(h && h->eng && n_nodes, "NULL argument");
    *n_nodes = h->eng->gameTreePriors(slot, max_nodes, priors, next_prior, next_pos);
  });
}

int coffee_match_game_tree_priors(coffee_match* h, int slot, int max_nodes, float* priors, float* next_prior,
                                  int32_t* next_pos, int* n_nodes) {
  return guarded([&] {
    need(h && h->eng && n_nodes, "NULL argument");
    *n_nodes = h->eng->gameTreePriors(slot, max_nodes, priors, next_prior, next_pos);
  });
}

int coffee_analysis_game_tree_priors(coffee_analysis* h, int slot, int max_nodes, float* priors, float* next_prior,
                                     int32_t* next_pos, int* n_nodes) {
  return guarded([&] {
    need(h && h->eng && n_nodes, "NULL argument");
    *n_nodes = h->eng->gameTreePriors(slot, max_nodes, priors, next_prior, next_pos);
  });
}

// ---- wide root noise and futile-visit pruning (rootsearch.h: the sequences the kernels run) ----

void coffee_root_search_params_default(coffee_root_search_params* p) {
  if(!p)
    return;
  p->wide_root_noise = 0.0f;  // searchparams.cpp: both off
  p->futile_visits_threshold = 0.0f;
}

int coffee_wide_root_noise(const coffee_root_search_params* p, uint64_t seed, uint32_t global_slot_or_stream,
                           uint32_t game_num, int32_t turn, uint32_t root_visits, int32_t pos, float prior,
                           float* smoothed_prior, float* bonus) {
  return guarded([&] {
    need(p != nullptr, "NULL argument");
    need(turn >= 0 && pos >= 0 && pos < MAX_P, "turn or pos out of range");
    const RootSearch r = toRootSearch(*p);
    float sm = prior, b = 0.0f;
    if(r.wide > 0.0f) {
      const uint64_t key = wideRootKey(gameStreamSeed(seed, global_slot_or_stream, game_num), turn, root_visits);
      b = wideBonus(r.wide, key, pos);
      sm = wideSmoothedPrior(r.wide, prior);
    }
    if(smoothed_prior)
      *smoothed_prior = sm;
    if(bonus)
      *bonus = b;
  });
}

int coffee_futile_visits(const coffee_root_search_params* p, float max_child_weight, float parent_weight_sum,
                         int64_t parent_visits, int64_t visits_left, int64_t edge_visits, int64_t child_visits,
                         float child_weight, int is_new, int* futile) {
  return guarded([&] {
    need(p && futile, "NULL argument");
    auto u32 = [](int64_t x) { return x <= 0 ? 0u : (x > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)x); };
    need(visits_left >= INT32_MIN && visits_left <= INT32_MAX, "visits_left out of range");
    const RootSearch r = toRootSearch(*p);
    *futile = 0;
    if(!(r.thr > 0.0f))
      return;
    // the kernels' own conversions: u32 visits, the visits left an i32 difference
    const float wpv = parent_weight_sum / (float)u32(parent_visits);
    const float left = (float)(int32_t)visits_left;
    *futile = is_new ? futileNew(r.thr, max_child_weight, wpv, left)
                     : futileChild(r.thr, max_child_weight, wpv, left, u32(edge_visits), u32(child_visits), child_weight);
  });
}

int coffee_selfplay_set_root_search(coffee_selfplay* h, const coffee_root_search_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setRootSearch(-1, *p);
  });
}

int coffee_analysis_set_root_search(coffee_analysis* h, const coffee_root_search_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setRootSearch(-1, *p);
  });
}

int coffee_match_set_root_search(coffee_match* h, int side, const coffee_root_search_params* p) {
  return guarded([&] {
    need(h && h->eng && p, "NULL argument");
    h->eng->setRootSearch(side, *p);
  });
}

// ---- parallel playouts per search (vloss.h: the sequence the kernels run) ----

int coffee_analysis_set_search_threads(coffee_analysis* h, int threads, float virtual_losses_per_thread) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    h->eng->setSearchThreads(threads, virtual_losses_per_thread);
  });
}

int coffee_analysis_search_threads_info(coffee_analysis* h, coffee_search_threads_info* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->searchThreadsInfo(*out);
  });
}

int coffee_analysis_round_paths(coffee_analysis* h, int slot, coffee_round_paths* out) {
  return guarded([&] {
    need(h && h->eng && out, "NULL argument");
    h->eng->roundPaths(slot, *out);
  });
}

int coffee_virtual_loss(float per_thread, uint32_t vl, int mover, float utility, float weight, float* u_out,
                        float* w_out) {
  return guarded([&] {
    need(mover == 1 || mover == 2, "mover must be 1 (black) or 2 (white)");
    need(per_thread > 0.0f && std::isfinite(per_thread), "per_thread must be finite and > 0");
    float u = utility, w = weight;
    virtualLossAdjust(per_thread, vl, mover, u, w);
    if(u_out)
      *u_out = u;
    if(w_out)
      *w_out = w;
  });
}

// ---- start positions (startpos.h: the thresholds and the pick the kernels run) ----

void coffee_start_positions_params_default(coffee_start_positions_params* p) {
  if(!p)
    return;
  p->prob = 0.0f;
  p->turn_weight_lambda = 0.0f;
  p->start_policy_init_area_prop = 0.0f;
}

int coffee_start_positions_check(int x, int y, int win_len, int n, const coffee_start_position* samples,
                                 int32_t* status_out, int32_t* info_out) {
  return guarded([&] {
    checkGeom(x, y, win_len);
    checkStartPositions(x, y, win_len, n, samples, status_out, info_out);
  });
}

int coffee_start_positions_thresholds(const coffee_start_position* samples, int n, float turn_weight_lambda,
                                      uint64_t* cum_out) {
  return guarded([&] { startPosThresholdsOf(samples, n, turn_weight_lambda, cum_out); });
}

int coffee_start_position_index(const uint64_t* cum, int n, uint64_t r, int* index) {
  return guarded([&] {
    need(cum && index && n >= 1, "start positions: NULL argument or n < 1");
    *index = startPosIndex(cum, n, r);
  });
}

int coffee_start_position_draws(uint64_t seed, uint32_t global_slot, uint32_t game_num, float prob,
                                const uint64_t* cum, int n, int* index, uint64_t* rng_counter) {
  return guarded([&] {
    need(index != nullptr, "NULL argument");
    need(n >= 0 && prob >= 0.0f && prob <= 1.0f, "start positions: n >= 0 and prob in [0, 1]");
    // startGame's stream: the seed, the two game-hash draws, then the start-position draws
    DRng rng{gameStreamSeed(seed, global_slot, game_num), 0};
    rng.next();
    rng.next();
    *index = startPosDraw(rng, prob, cum, n);
    if(rng_counter)
      *rng_counter = rng.ctr;
  });
}

int coffee_start_position_pick(uint64_t seed, uint32_t global_slot, uint32_t game_num, float prob,
                               const uint64_t* cum, int n, int* index) {
  return coffee_start_position_draws(seed, global_slot, game_num, prob, cum, n, index, nullptr);
}

int coffee_selfplay_set_start_positions(coffee_selfplay* h, const coffee_start_position* samples, int n,
                                        const coffee_start_positions_params* params) {
  return guarded([&] {
    need(h && h->eng && params, "NULL argument");
    h->eng->setStartPositions(samples, n, *params);
  });
}

int coffee_match_set_start_positions(coffee_match* h, const coffee_start_position* samples, int n,
                                     const coffee_start_positions_params* params) {
  return guarded([&] {
    need(h && h->eng && params, "NULL argument");
    h->eng->setStartPositions(samples, n, *params);
  });
}

int coffee_selfplay_start_position_games(coffee_selfplay* h, uint64_t* games) {
  return guarded([&] {
    need(h && h->eng && games, "NULL argument");
    *games = h->eng->startPositionGames();
  });
}

int coffee_match_start_position_games(coffee_match* h, uint64_t* games) {
  return guarded([&] {
    need(h && h->eng && games, "NULL argument");
    *games = h->eng->startPositionGames();
  });
}

int coffee_debug_cdf_table(int x, int y, int win_len, float* out) {
  return guarded([&] {
    need(out != nullptr, "NULL argument");
    checkGeom(x, y, win_len);
    DTables t = buildTables(x, y, win_len);
    memcpy(out, t.cdf, sizeof(float) * CDF_SIZE);
  });
}

int coffee_debug_zobrist(int x, int y, int win_len, uint64_t* board, uint64_t* board2, uint64_t* player,
                         uint64_t* init, uint64_t* game_over) {
  return guarded([&] {
    need(board && board2 && player && init && game_over, "NULL argument");
    checkGeom(x, y, win_len);
    DTables t = buildTables(x, y, win_len);
    memcpy(board, t.zBoard, sizeof(uint64_t) * t.A * 3 * 2);
    memcpy(board2, t.zBoard2, sizeof(uint64_t) * t.A * 4 * 2);
    memcpy(player, t.zPlayer, sizeof(t.zPlayer));
    memcpy(init, t.zInit, sizeof(t.zInit));
    memcpy(game_over, t.zGameOver, sizeof(t.zGameOver));
  });
}

int coffee_selfplay_enable_timing(coffee_selfplay* h, int enable) {
  return guarded([&] {
    need(h && h->eng, "NULL handle");
    need(enable >= 0, "enable must be >= 0");
    h->eng->setTiming(enable);
  });
}

int coffee_selfplay_timed_nn_evals(coffee_selfplay* h, uint64_t* evals) {
  return guarded([&] {
    need(h && h->eng && evals, "NULL argument");
    *evals = h->eng->timedNNEvals();
  });
}

int coffee_selfplay_kernel_time(coffee_selfplay* h, int which, double* ms, uint64_t* launches) {
  return guarded([&] {
    need(h && h->eng && ms && launches, "NULL argument");
    h->eng->kernelTime(which, *ms, *launches);
  });
}

}  // extern "C"
