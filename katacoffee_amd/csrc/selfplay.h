// Host self-play engine (selfplay.cpp) behind coffee_selfplay_*, and the same engine in
// two-network match mode behind coffee_match_*.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "../../include/katacoffee.h"
#include "engine.h"
#include "search.h"

namespace kc {

SP toSP(const coffee_search_params& p);
// Checks the ranges (throws std::invalid_argument naming the setting; NaN is out of range)
// and converts.
Unc toUnc(const coffee_uncertainty_params& p);
// The device block of coffee_exploration_params; throws std::invalid_argument outside the
// reference's ranges (setup.cpp:453-470, :520-537), for a non-finite value and for prior 0 with
// scale > 0.
Expl toExpl(const coffee_exploration_params& p);
// The device block of coffee_root_search_params; throws std::invalid_argument outside the
// reference's ranges (wideRootNoise [0, 5]; futileVisitsThreshold 0 or [0.01, 1]) and for a
// non-finite value.
RootSearch toRootSearch(const coffee_root_search_params& p);
// Start positions: the parameters' ranges; the thresholds of a table on the host (startpos.h);
// the check kernel on a host table at a geometry.  Each throws std::invalid_argument naming
// the setting or the first bad sample.
void validateStartPosParams(const coffee_start_positions_params& p);
void startPosThresholdsOf(const coffee_start_position* samples, int n, float lambda, uint64_t* cum);
void checkStartPositions(int x, int y, int winLen, int n, const coffee_start_position* samples, int32_t* status,
                         int32_t* info);
// Checks a match config without touching the device (throws std::invalid_argument naming
// the offending setting): geometry, and the settings match play rejects because they keep
// a tree across moves or exist only to make training rows.
void validateMatchConfig(const coffee_match_config& c);
// The same for the per-side options of coffee_match_create2 (nullptr: nothing to check): each
// side's parameters as validateMatchConfig and the engine's own range checks see them, its
// uncertainty parameters, the game-level fields against c.search, share_net's equal model
// paths, and the node pool against each side's max_visits.  The message names side and field.
void validateMatchOptions(const coffee_match_config& c, const coffee_match_options* o);
// The node pool of a config: node_cap (0: max(2048, 3 * maxVisits)) rounded up to 64.
int nodeCapFor(int nodeCap, int maxVisits);
// The same for an analysis config: geometry, num_slots, query_capacity, max_pv_len, and the
// settings of validateMatchConfig plus init_games_with_policy.
void validateAnalysisConfig(const coffee_analysis_config& c);
// A query's host-side checks at board x * y (throws std::invalid_argument naming the field):
// num_moves in 0..x*y, every move < 4*x*y, max_visits >= 0.
void validateAnalysisQuery(int x, int y, const coffee_analysis_query& q);
// A query's root restriction at board x * y: mode 0..2, no bit at a position >= 4*x*y, a set
// only where the board's positions fit its words.
void validateAnalysisRestrict(int x, int y, uint64_t id, const coffee_analysis_restrict& r);

class SelfplayEngine {
 public:
  explicit SelfplayEngine(const coffee_selfplay_config& c) : SelfplayEngine(c, nullptr) {}
  // Match mode: net 0 (baseline) against net 1 (candidate); a NULL model path is the stand-in
  // opts (coffee_match_create2; nullptr: none): per-side search settings, one shared net
  explicit SelfplayEngine(const coffee_match_config& c, const coffee_match_options* opts = nullptr);
  // Analysis mode (DESIGN.md "Analysis"): the slots search queued positions instead of games
  explicit SelfplayEngine(const coffee_analysis_config& c);
  ~SelfplayEngine();
  void step(int rounds, hipStream_t st);
  void sync();
  // Uncertainty weighting of the evaluations, for every net of the engine.  Only before the
  // first round (analysis: and the first query); throws std::invalid_argument afterwards or
  // for out-of-range values, without touching the device.
  void setUncertainty(const coffee_uncertainty_params& p);
  // side: -1 on an engine without per-side settings, 0 / 1 on one with them
  void setExploration(int side, const coffee_exploration_params& p);
  void setRootSearch(int side, const coffee_root_search_params& p);
  // Start positions: checks the parameters and every sample (kStartPosCheck),
  // builds the thresholds and uploads both once the engine stream is idle; between steps at any time.
  // Throws std::invalid_argument (naming the first bad sample) with the engine untouched.
  // Before the first round every slot's first game is started again.  n = 0: off.
  void setStartPositions(const coffee_start_position* samples, int n, const coffee_start_positions_params& p);
  uint64_t startPositionGames();  // games started from the table so far
  void stats(coffee_selfplay_stats& out);
  void matchStats(coffee_match_stats& out);
  // Analysis mode: queries into the device ring on the engine stream (returns how many fit),
  // finished results out of it (returns their number), the counters.
  // rs (nullptr: none): the queries' root restrictions; rootInfo / policy (nullptr: skipped): the
  // results' used symmetries and masked-move counts, and with include_policy the root policies
  int analysisSubmit(const coffee_analysis_query* q, const coffee_analysis_restrict* rs, int n);
  int analysisDrain(int max, coffee_analysis_result* header, coffee_analysis_move* moves,
                    coffee_analysis_root_info* rootInfo = nullptr, float* policy = nullptr);
  // Root restrictions: only before the first submitted query.
  void setRootOptions(const coffee_analysis_root_options& o);
  void analysisStats(coffee_analysis_stats& out);
  // Parallel playouts per search: only while the engine holds no query.  Throws
  // std::invalid_argument, the engine untouched, for a value out of range or num_slots x threads
  // past the batch cap of one network launch.
  void setSearchThreads(int threads, float perThread);
  void searchThreadsInfo(coffee_search_threads_info& out);
  void roundPaths(int slot, coffee_round_paths& out);
  int drain(int maxRows, uint8_t* bin, float* glob, int16_t* pol, float* gt, int8_t* val, int32_t* meta);
  // header [g][4]; match mode [g][5], the candidate's colour last
  int drainGames(int maxGames, int32_t* header, uint8_t* moves);
  // Stream-ordered row hand-off (no host synchronisation): packs every pending row into
  // dst (device, >= rowCap rows), their count into *countOut (host, valid once the
  // engine stream passes this point) and empties the buffer.
  void stageRows(uint8_t* dst, int maxRows, unsigned long long* countOut, bool discardGames);
  hipStream_t stream() const { return stream_; }
  // Replaces the network for all subsequent rounds (all games: switchNetsMidGame).
  void setModel(const char* path);
  // The same from a CFNN image in host memory (weights broadcast from another rank).
  void setModelBytes(const void* data, size_t bytes);
  void gameInfo(int slot, int64_t* info);
  int gameTree(int slot, int maxNodes, uint32_t* nodes, uint32_t* edges);
  int gameTreePriors(int slot, int maxNodes, float* priors, float* nextPrior, int32_t* nextPos);
  void rootPolicy(int slot, float* out);
  // every = 0: off; N: time every N-th launch of each kernel group (HIP events;
  // each event pair costs a few microseconds of stream gap, so sampling keeps
  // the timed run representative)
  void setTiming(int every) { timingEvery_ = every > 0 ? every : 0; }
  void kernelTime(int which, double& ms, uint64_t& launches);
  uint64_t timedNNEvals();
  const SearchDev& dev() const { return hd_; }
  bool nnFused() const { return nets_[0].nn && nets_[0].nn->fused(); }

 private:
  struct PendingTiming {
    int which;
    hipEvent_t a, b;
  };
  void switchModel(const ModelHost& m);
  void timed(int which, hipStream_t st, const std::function<void()>& f, bool on);
  void timedKernel(int which, bool on, const std::function<void(hipEvent_t, hipEvent_t)>& f);
  bool sampleNow(int which) { return timingEvery_ > 0 && groupLaunches_[which]++ % (uint64_t)timingEvery_ == 0; }
  hipEvent_t takeEvent();
  void resolveTiming();
  std::vector<PendingTiming> pending_;
  std::vector<hipEvent_t> evPool_;
  // matchPaths: the two model paths of match mode (self-play: nullptr); matchOpts: its options
  SelfplayEngine(const coffee_selfplay_config& c, const char* const* matchPaths,
                 const coffee_match_options* matchOpts = nullptr);
  static coffee_selfplay_config matchBase(const coffee_match_config& c, const coffee_match_options* o);
  static coffee_selfplay_config analysisBase(const coffee_analysis_config& c);
  // analysis: queries submitted / results drained so far
  uint64_t aSubmitted_ = 0, aDrained_ = 0;
  bool aIncludePolicy_ = false;
  const DTables* T_ = nullptr;
  // Per-network state: self-play holds one network, match play two (each resolves its
  // precision and runs its audit on its own batches).
  struct Net {
    std::unique_ptr<NNEngine> nn;      // null: the stand-in network
    std::unique_ptr<ModelHost> model;  // the network's model (rebuilt on an audit switch)
    float* auditOut = nullptr;         // device [G][P+4]: the accurate instance's rows
    unsigned* auditMax = nullptr;      // device: largest difference so far (float bits)
    uint64_t nnLaunches = 0;
    uint64_t audits = 0;
    float auditSeen = 0.0f;            // largest difference read back so far
    int auditSwitches = 0;
  };
  Net nets_[2];
  int numNets_ = 1;
  // one network launch (and its audit, when due) of net n on the list idx / count
  void forwardNet(int n, const int32_t* count, const int32_t* idx, hipStream_t st, hipEvent_t a, hipEvent_t b);
  SearchDev hd_;
  SearchDev* dd_ = nullptr;
  std::vector<void*> owned_;
  hipStream_t stream_ = nullptr;
  int commitInterval_ = 8;
  int xLen_ = 0, yLen_ = 0, winLen_ = 0;
  int nnPath_ = 0;  // NNPath of the network (kept across hot reloads)
  int userCap_ = 0;          // coffee_selfplay_config.nn_batch_cap (0 = the network's default)
  int enginesPerDevice_ = 1; // engines sharing the device's default fused batch cap
  int cus_ = 1;              // compute units of the device
  int nnCapFor(int G) const;
  // network rows of a round: one per slot, or with parallel playouts one per slot and descent
  int rows() const { return hd_.G * std::max(1, (int)hd_.wideK); }
  size_t rowsAllocated_ = 0;                  // rows the network batch arrays hold
  unsigned long long* vlCount_ = nullptr;     // device: launchVirtualLossCount's sum
  int32_t modelGen_ = 0;  // hot reloads so far
  uint64_t rounds_ = 0;
  bool commitReset_ = false;  // a commit ran: the next kSelect zeroes the commit count
  uint64_t rowsDrained_ = 0;
  int timingEvery_ = 0;
  // kernel timing slots: 0 select, 1 network, 2 backup, 3 commit, 4 backup + next select (fused)
  uint64_t groupLaunches_[5] = {0, 0, 0, 0, 0};
  double kernelMs_[5] = {0, 0, 0, 0, 0};
  uint64_t kernelLaunches_[5] = {0, 0, 0, 0, 0};
  // a round's backup and the next round's selection run as one kernel unless a commit
  // comes between them -- with the fast fused network or the stand-in (measured: with the
  // corrected network, which bounds the round, the longer-lived search waves delay its
  // workgroups: 202 vs 161 us).  COFFEE_FUSED_ROUNDS=0: never, 1: always (same results)
  int fuseRounds_ = -1;  // -1 auto, 0 never, 1 always
  bool fuseNow() const;
  // after a fused round the pending selections are completed and the round's cache tags
  // cleared by the compaction's own dispatch (kCompact resolve phase) instead of a separate
  // kResolve launch; COFFEE_SEPARATE_RESOLVE=1 keeps the separate launch (same results)
  bool resolveInCompact_ = true;
  // Audit of the default precision on self-play's own positions: every
  // auditEvery_-th network launch of an engine whose default precision resolved to the
  // corrected instance is re-evaluated (its first NN_AUDIT_ROWS rows) on the accurate
  // instance; sync() -- every stats / drain / game-record call -- reads the largest
  // difference so far and, past auditTol_ (NNEngine::NN_AUTO_TOL), rebuilds the network
  // at the accurate precision (same model; the NN cache is cleared).  The switch happens
  // only at those host synchronisation points, so runs stay reproducible.
  // COFFEE_NN_AUDIT_EVERY (0 = off) and COFFEE_NN_AUDIT_TOL override the defaults.
  void auditCheck();
  int auditEvery_ = 128;
  float auditTol_ = NNEngine::NN_AUTO_TOL;
};

}  // namespace kc
