/* katacoffee.h — C ABI of the MI355X Coffee self-play engine (libkatacoffee.so).
 *
 * This is the drop-in boundary of SURVEY.md §8(b): the in-process surface that
 * replaces the reference's rules / encoder / NN-backend / self-play hot path.
 * Every entry point:
 *   - is extern "C", takes plain pointers and sizes, never throws;
 *   - returns 0 on success and a negative COFFEE_E* code on failure, with the
 *     message in coffee_last_error() (thread-local) — the reference reports the
 *     same failures as C++ StringError exceptions (eigenbackend.cpp:1602-1605);
 *   - takes DEVICE pointers for bulk data unless the parameter says "host",
 *     and an optional hipStream_t (`stream`, NULL = the default stream).
 * Handles are single-thread objects, like NeuralNet::ComputeHandle
 * (nninterface.h:18-20) and Search (search.h:159-165); use one handle per GPU.
 *
 * Board geometry: X columns x Y rows, 2 <= X, Y <= 10; cell = y*X + x; A = X*Y.
 * Move encoding ("pos"): pos = dir*A + cell, dir 0=N 1=W 2=NW 3=NE (board.h:41-47);
 * P = 4A.  Colours: 0 empty, 1 black, 2 white.  Player 1 moves first.
 * lastDir 4 = NONE (no previous move), lastCell -1 = none.
 */
#ifndef KATACOFFEE_H
#define KATACOFFEE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COFFEE_OK 0
#define COFFEE_EINVAL (-1)   /* bad argument / unsupported geometry or model */
#define COFFEE_EHIP (-2)     /* HIP runtime error */
#define COFFEE_EIO (-3)      /* file I/O or format error */
#define COFFEE_EINTERNAL (-4)

#define COFFEE_NUM_SPATIAL 15 /* V1 planes (README "V1", SPEC a6) */
#define COFFEE_NUM_GLOBAL_TARGETS 64

/* Last error message of the calling thread ("" if none). */
const char* coffee_last_error(void);
/* ABI version (major*100 + minor). */
int coffee_abi_version(void);

/* ---- device memory helpers (so callers need no HIP headers) ---- */
int coffee_device_count(int* count);
int coffee_set_device(int device);
/* Compute units of `device` (the fused network runs one workgroup per CU: a host that
   runs several self-play engines on one device splits cus x 8 rows of batch cap
   between them, as the CLI does for numNNServerThreadsPerModel). */
int coffee_device_compute_units(int device, int* cus);
int coffee_malloc(void** dev_ptr, uint64_t bytes);
int coffee_free(void* dev_ptr);
/* kind: 0 host->device, 1 device->host, 2 device->device */
int coffee_memcpy(void* dst, const void* src, uint64_t bytes, int kind);
int coffee_synchronize(void);

/* ---- rules (replaces Board::isLegal board.cpp:185-227,
 *      Board::playMoveAssumeLegal board.cpp:427-435 + BoardHistory::makeBoardMoveAssumeLegal
 *      boardhistory.cpp:157-176, Board::maxConsecutives board.cpp:315-335,
 *      Board pos_hash board.cpp:134-178, GraphHash::getStateHash graphhash.cpp:3-34) ---- */

/* n positions.  cells [n][A] u8 colours; last_cell/last_dir [n] int8; pla [n] u8.
 * legal  [n][P] u8 (1 = legal move for pla)        (out)
 * has_legal [n] u8 (0 = no legal move: SPEC B16 draw) (out) */
int coffee_rules_batch(int x, int y, int win_len, int n, const uint8_t* cells, const int8_t* last_cell,
                       const int8_t* last_dir, const uint8_t* pla, uint8_t* legal, uint8_t* has_legal, void* stream);

/* Plays move[i] (pos, assumed legal) for pla[i].  Outputs:
 * out_cells [n][A]; finished/winner [n] u8 (winner 0 = none/draw); max_run [n] i32
 * (longest run through the move); pos_hash [n][2] u64 (Board::pos_hash after);
 * state_hash [n][2] u64 (transposition key: pos_hash ^ next player ^ last move ^ game over). */
int coffee_play_batch(int x, int y, int win_len, int n, const uint8_t* cells, const int8_t* last_cell,
                      const int8_t* last_dir, const uint8_t* pla, const int32_t* move, uint8_t* out_cells,
                      uint8_t* finished, uint8_t* winner, int32_t* max_run, uint64_t* pos_hash,
                      uint64_t* state_hash, void* stream);

/* ---- V1 encoder (replaces NNInputs::fillRowV1 nninputs.cpp:508-657 with SPEC a6,
 *      symmetry SymmetryHelpers nninputs.cpp:252-433) ---- */

/* hist_cell/hist_dir [n][5]: the last five moves, [0] most recent (-1 / 4 = none).
 * sym [n] in 0..7 (bit0 flip y, bit1 flip x, bit2 transpose; transpose ignored when X != Y).
 * packed [n][ceil(15A/64)] u64: bit i = plane*A + symcell      (out, required)
 * planes [n][15][A] f32 (NCHW, symmetric frame)                  (out, optional: NULL)
 * The global input is the single value win_len. */
int coffee_encode_batch(int x, int y, int win_len, int n, const uint8_t* cells, const int8_t* hist_cell,
                        const int8_t* hist_dir, const uint8_t* pla, const int32_t* sym, uint64_t* packed,
                        float* planes, void* stream);

/* ---- network (replaces the NeuralNet:: backend interface nninterface.h:31-171:
 *      loadModelFile / createComputeHandle / getOutput / free*) ---- */

typedef struct coffee_nn coffee_nn;

/* Writes a seeded random-init CFNN model file ("b6c96", "b10c128", "b18c384nbt",
 * "b2c32", "b2c32nbt"; modelconfigs.py:129/156/887). */
int coffee_model_write_random(const char* arch, uint64_t seed, const char* path /* host */);
/* FLOPs per evaluation (2 x MACs) of a CFNN model at area A. */
int coffee_model_flops(const char* path, int area, double* flops);

/* Loads a CFNN model and prepares device weights for boards X x Y with win length W
 * (NeuralNet::loadModelFile + createComputeHandle, nninterface.h:42-109).
 * coffee_nn_create = coffee_nn_create2(..., COFFEE_NN_DEFAULT, ...). */
int coffee_nn_create(const char* model_path, int x, int y, int win_len, coffee_nn** out);
/* precision (the reference's useFP16 switch, nninterface.h:76-88; its default, Auto,
 * setup.cpp:240-248, maps here to the path that meets the north-star 1e-3 of fp32):
 *   COFFEE_NN_DEFAULT       (0) the 1e-3 path: where the fused kernel covers the net (b6c96
 *                           @ 5x5), CORRECTED if a load-time calibration batch (corrected vs
 *                           accurate on 256 seeded positions) differs by at most 2.5e-4 and
 *                           flags no board, else ACCURATE; the layered split (ACCURATE)
 *                           kernels for every other net (coffee_nn_precision reports it)
 *   COFFEE_NN_ACCURATE      fp16 hi/lo operand pairs on three MFMAs (the fused kernel's
 *                           split instance where it covers the net, the layered kernels
 *                           otherwise): logits within ~1e-5 of the fp32 (Eigen-semantics) forward
 *   COFFEE_NN_FAST_LAYERED  fp16 operands on the layered kernels (any architecture)
 *   COFFEE_NN_CORRECTED     fp16 products plus the two fp16-rounding cross terms on
 *                           block-scaled e4m3 MFMAs (twice the fp16 MFMA work): the weights'
 *                           e4m3 operands carry one power-of-two exponent per convolution
 *                           (its largest |w| lands in (224, 448], so no weight saturates);
 *                           activations are unscaled, and a board with a convolution input
 *                           past e4m3's 448 is flagged and re-evaluated on the ACCURATE
 *                           instance in a second launch.  A product is good to ~2^-14, so
 *                           the error grows with the logits: 7e-4 of fp32 on a net trained
 *                           200 steps (logits ~20), ~1e-3 after 1000 -- not
 *                           a 1e-3 path for every net, hence DEFAULT's calibration.  The
 *                           fused kernel where it covers the net, else as ACCURATE
 *   COFFEE_NN_ACCURATE_NB2  ACCURATE on the 2-board bordered fused instance (A/B reference
 *                           of the borderless 5-board one; same results bit for bit)
 *   COFFEE_NN_FAST          fp16 MFMA operands, f32 accumulation and residual trunk (the
 *                           fused single-launch kernel where it covers the net, the layered
 *                           kernels otherwise): ~1e-3 of the largest logit off fp32, which
 *                           misses the 1e-3 absolute bound on trained nets */
#define COFFEE_NN_DEFAULT 0
#define COFFEE_NN_ACCURATE 1
#define COFFEE_NN_FAST_LAYERED 2
#define COFFEE_NN_CORRECTED 3
#define COFFEE_NN_ACCURATE_NB2 4
#define COFFEE_NN_FAST 5
int coffee_nn_create2(const char* model_path, int x, int y, int win_len, int precision, coffee_nn** out);
/* 1 when the handle runs the fused single-launch kernel, 0 for the layered kernels. */
int coffee_nn_is_fused(coffee_nn* h, int* fused);
/* The precision the handle runs (COFFEE_NN_*, COFFEE_NN_DEFAULT resolved: CORRECTED, or
 * ACCURATE when the corrected instance's logits on a fixed calibration batch -- 256
 * positions of seeded random legal play -- differ from the accurate instance's by more than
 * 2.5e-4, a quarter of the north-star bound; ACCURATE / FAST_LAYERED on the layered kernels)
 * and that calibration difference (*calib_err, 0 when no check ran; may be NULL). */
int coffee_nn_precision(coffee_nn* h, int* precision, float* calib_err);
/* in: packed V1 rows [n][ceil(15A/64)] (coffee_encode_batch layout);
 * out: [n][P+4] f32 = policy logits [4][A] (symmetric frame, dir-major), value logits
 * (win, loss) from the side to move, misc[2].  fp16 MFMA operands (see precision),
 * f32 accumulation. */
int coffee_nn_forward(coffee_nn* h, int n, const uint64_t* in, float* out, void* stream);
/* NeuralNet::getOutput's contract (eigenbackend.cpp:1776-1796): as coffee_nn_forward, with
 * sym [n] i32 (device) = the symmetry each row was encoded with (coffee_encode_batch's
 * sym); the policy logits come back in the CANONICAL frame, the inverse symmetry applied
 * per SPEC B12 (cells un-flipped / un-transposed and the directions mapped back: a one-axis
 * flip swaps NW<->NE, a transpose swaps N<->W), as copyOutputsWithSymmetry does.  Value
 * logits (win, loss; side to move) and misc[2] are symmetry-free and unchanged.  The
 * NNEvaluator-side post-processing (legal mask, softmax, white perspective;
 * nneval.cpp:702-844) stays with the caller, as in the reference. */
int coffee_nn_forward2(coffee_nn* h, int n, const uint64_t* in, const int32_t* sym, float* out, void* stream);
int coffee_nn_destroy(coffee_nn* h);

/* The deterministic stand-in network (oracle fakeNet), same I/O as coffee_nn_forward. */
int coffee_fake_net(int x, int y, int win_len, int n, const uint64_t* in, float* out, void* stream);

/* ---- self-play engine (replaces Play::runGame play.cpp:1146-1701 driving
 *      Search::runWholeSearch search.cpp:361-509 and TrainingWriteBuffers
 *      trainingwrite.cpp:316-565 for numGameThreads games) ---- */

/* SearchParams (searchparams.h) restricted to Coffee self-play; defaults =
 * cpp/configs/training/selfplay1.cfg with benchmark settings. */
typedef struct coffee_search_params {
  int32_t max_visits;
  float cpuct_exploration, cpuct_exploration_log, cpuct_exploration_base;
  float fpu_reduction_max, root_fpu_reduction_max, fpu_loss_prop, root_fpu_loss_prop;
  int32_t fpu_parent_weight_by_visited_policy;
  float fpu_parent_weight_by_visited_policy_pow;
  float value_weight_exponent;
  int32_t root_noise_enabled;
  float root_dirichlet_noise_total_concentration, root_dirichlet_noise_weight;
  float root_policy_temperature, root_policy_temperature_early;
  float root_desired_per_child_visits_coeff;
  int32_t root_num_symmetries_to_sample;
  float chosen_move_temperature, chosen_move_temperature_early, chosen_move_temperature_halflife;
  float chosen_move_subtract, chosen_move_prune;
  int32_t use_lcb_for_selection;
  float lcb_stdevs, min_visit_prop_for_lcb;
  float subtree_value_bias_factor, subtree_value_bias_weight_exponent, subtree_value_bias_free_prop;
  int32_t use_graph_search;
  /* PlaySettings (playsettings.cpp): per-move search limits (getSearchLimitsThisMove
   * play.cpp:871-1004) and row weighting (play.cpp:1470-1697).  Defaults are the
   * benchmark mode of SURVEY 8d (all off); selfplay1.cfg values in comments. */
  float cheap_search_prob;           /* 0.75 */
  int32_t cheap_search_visits;       /* 100 */
  float cheap_search_target_weight;  /* 0.0 */
  int32_t reduce_visits;             /* 1 */
  float reduce_visits_threshold;     /* 0.9 */
  int32_t reduce_visits_threshold_lookback; /* 3 */
  int32_t reduced_visits_min;        /* 100 */
  float reduced_visits_weight;       /* 0.1 */
  float policy_surprise_data_weight; /* 0.5 */
  float value_surprise_data_weight;  /* 0.1 */
  /* opening moves sampled from the raw policy before the searched game
   * (initializeGameUsingPolicy playutils.cpp:147-176) */
  int32_t init_games_with_policy;    /* 1 */
  float policy_init_area_prop;       /* 0.04: mean number of moves / board area */
  float policy_init_area_temperature;/* 1.0 */
  /* forks (Play::maybeForkGame play.cpp:1741-1840): after a game, with these
   * probabilities the slot's next game starts from a replayed position of it plus the
   * best (by the value head) of a few random legal moves */
  float early_fork_game_prob;            /* 0.04 */
  float early_fork_game_expected_move_prop; /* 0.025 */
  float fork_game_prob;                  /* 0.01 */
  int32_t fork_game_min_choices;         /* 3 */
  int32_t early_fork_game_max_choices;   /* 12 */
  int32_t fork_game_max_choices;         /* 36 */
  /* side positions (play.cpp:1328-1345, :1576-1662): after a searched move, with this
   * probability a refutation position (the root policy's alternative to the played
   * move) is queued and searched after the game; one row each */
  float side_position_prob;              /* 0.02 */
  /* tree positions (recordTreePositions play.cpp:710-860, :1347-1361, :1612-1628): after
   * a searched move (or side position), positions of its search tree up to 5 moves deep
   * reached only through the mover's most-visited moves, from nodes with at least
   * record_tree_threshold visits, are written as side rows with weight
   * record_tree_target_weight (<= 1).  PlaySettings fields with these defaults
   * (playsettings.cpp:14); the reference's selfplay config loader does not read them */
  int32_t record_tree_positions;         /* 0 */
  int32_t record_tree_threshold;         /* 0 */
  float record_tree_target_weight;       /* 0.0 */
} coffee_search_params;

void coffee_search_params_default(coffee_search_params* p);

typedef struct coffee_selfplay_config {
  int32_t x, y, win_len;
  int32_t num_games;     /* concurrent games on this device (numGameThreads) */
  int32_t node_cap;      /* per-game node pool; 0 = max(2048, 3*max_visits) */
  int32_t row_capacity;  /* device row buffer capacity; 0 = 4*num_games*A */
  uint64_t seed;         /* run seed (gameSeedBase) */
  int32_t slot_base;     /* global index of slot 0 (rank * num_games) */
  int32_t use_fake_net;  /* 1 = coffee_fake_net instead of the model */
  int32_t commit_interval; /* rounds between move-commit launches (0 = 8); 1 commits in
                              the round the root reaches max_visits, like the oracle */
  const char* model_path;/* CFNN model (host string), ignored with use_fake_net */
  coffee_search_params search;
  int32_t nn_cache_log2; /* NN evaluation cache entries = 2^nn_cache_log2 (selfplay1.cfg
                            nnCacheSizePowerOfTwo = 21); 0 disables (SPEC a7) */
  int32_t nn_batch_cap;  /* rows per network launch; leaves past it wait for the next round,
                            ahead of new ones.  0 = one full wave of network workgroups
                            (compute units x 8 boards: 2048 on MI355X, / engines_per_device)
                            for the fused kernel, unbounded for the layered kernels */
  int32_t nn_precision;  /* COFFEE_NN_DEFAULT (0: the 1e-3 path) / _CORRECTED / _ACCURATE /
                            _FAST / _FAST_LAYERED */
  int32_t start_stagger; /* > 0: each slot idles a seeded number of rounds in [0, start_stagger)
                            before its first game (benchmarks: spreads game ends over the
                            run); 0 = all games start in round 0 */
  int32_t engines_per_device; /* engines sharing this device (the CLI's numNNServerThreadsPerModel
                            engines on one GPU); with nn_batch_cap 0 a fused network's default
                            cap (one wave of network workgroups) is split between them, also
                            after a hot reload that changes the network path; 0 or 1 = alone */
} coffee_selfplay_config;

typedef struct coffee_selfplay coffee_selfplay;

typedef struct coffee_selfplay_stats {
  uint64_t rounds;          /* select -> NN -> backup rounds run */
  uint64_t playouts;        /* completed playouts (runSinglePlayout true) */
  uint64_t nn_evals;        /* network rows evaluated */
  uint64_t moves;           /* moves committed */
  uint64_t games_finished;
  uint64_t rows_written;    /* rows produced so far (drained + pending) */
  uint64_t rows_pending;    /* rows on the device not yet drained */
  uint64_t rows_dropped;    /* rows lost to a full row buffer (drain more often) */
  uint64_t games_dropped;   /* game records lost to a full record buffer (2 x num_games) */
  uint64_t errors;          /* device invariant violations (node pool exhausted, no move
                               candidate); nonzero makes stats return COFFEE_EINTERNAL */
  uint64_t tree_levels;     /* tree levels descended by all playouts (path nodes) */
  uint64_t tree_children;   /* children scanned at those path nodes (select reads each
                               path node and its k children; backup re-aggregates them) */
  uint64_t errors_node_pool; /* slots whose node pool ran out (part of errors) */
  uint64_t errors_edge_pool; /* slots whose edge pool (children past 16 per node) ran out */
  uint64_t edge_pool_peak;  /* largest edge-pool use of any slot so far (entries) */
  uint64_t edge_pool_cap;   /* edge-pool entries per slot and buffer */
  uint64_t nn_precision;    /* the precision the network runs (coffee_nn_precision; 0 = stand-in net) */
  /* Default precision on self-play's own positions: every 128th network launch of an engine
   * running the corrected instance re-evaluates its first 256 rows on the accurate one; the
   * largest |logit| difference is read at every stats / drain call and, past 2.5e-4, the
   * engine switches to the accurate instance for the rest of the run (the same model). */
  uint64_t nn_audits;         /* audited launches so far */
  uint64_t nn_audit_switches; /* switches to the accurate instance (0 or 1 per model) */
  double nn_audit_max_diff;   /* largest difference seen so far (0 before the first audit) */
} coffee_selfplay_stats;

int coffee_selfplay_create(const coffee_selfplay_config* cfg, coffee_selfplay** out);
/* Runs `rounds` rounds (one playout or root evaluation per game per round) on `stream`
 * (NULL = the engine's own stream).  Asynchronous: call coffee_selfplay_sync. */
int coffee_selfplay_step(coffee_selfplay* h, int rounds, void* stream);
int coffee_selfplay_sync(coffee_selfplay* h);
int coffee_selfplay_stats_get(coffee_selfplay* h, coffee_selfplay_stats* out);

/* Copies up to max_rows finished rows to HOST buffers and removes them from the device
 * buffer (trainingwrite.cpp:185-205 shapes; 5x5: pb = ceil(A/8) = 4):
 *   bin   [r][15][pb] u8   binaryInputNCHWPacked (big-endian bits, packBits :218-232)
 *   glob  [r][1]   f32     globalInputNC
 *   pol   [r][2][P] i16    policyTargetsNCMove
 *   gtgt  [r][64]  f32     globalTargetsNC
 *   value [r][5][A] i8     valueTargetsNCHW
 *   meta  [r][4]   i32     (slot, game number, turn, num moves) — not part of the .npz
 * Any output pointer may be NULL.  *n_out = rows copied. */
int coffee_selfplay_drain_rows(coffee_selfplay* h, int max_rows, uint8_t* bin, float* glob, int16_t* pol,
                               float* gtgt, int8_t* value, int32_t* meta, int* n_out);
/* Copies up to max_games finished-game records to HOST buffers and removes them
 * (the moves the reference's SGF writer prints, sgf.cpp:1526-1700 / selfplaymanager.cpp:350):
 *   header [g][4] i32  (slot, game number, number of moves, winner 0 draw / 1 black / 2 white)
 *   moves  [g][A][2] u8 (cell = y*x_len + x, direction 0..3 = N, W, NW, NE; 0xFF past the end)
 * Either output pointer may be NULL.  *n_out = records copied. */
int coffee_selfplay_drain_games(coffee_selfplay* h, int max_games, int32_t* header, uint8_t* moves, int* n_out);
/* Device-resident row hand-off for multi-GPU writers (the RCCL gather of SURVEY 8e;
 * trainingwrite.cpp:774-937 writes the rows afterwards).  Enqueued on the engine's own
 * stream, returns at once: every pending row is packed into dst (DEVICE memory,
 * [max_rows][coffee_row_bytes] u8, one record per row = bin, glob, pol, gtgt, value,
 * meta of coffee_selfplay_drain_rows back to back; max_rows >= the engine's row
 * capacity), the number of rows is copied to *count (HOST memory, pinned for an
 * asynchronous copy; valid once the engine stream has passed this call: wait on an
 * event recorded on coffee_selfplay_stream) and the engine's row buffer is emptied.
 * flags COFFEE_STAGE_DISCARD_GAMES: also drop the finished-game records (a caller that
 * writes no SGF).  The next steps may be enqueued before the rows are consumed. */
#define COFFEE_STAGE_DISCARD_GAMES 1
int coffee_selfplay_stage_rows(coffee_selfplay* h, void* dst, int max_rows, uint64_t* count, int flags);
int coffee_selfplay_row_capacity(coffee_selfplay* h, int* rows);
int coffee_row_bytes(int x, int y, int* bytes);
/* The engine's HIP stream (hipStream_t), for callers that order their own work
 * (events, copies, collectives) against the engine's. */
int coffee_selfplay_stream(coffee_selfplay* h, void** stream);
/* Replaces the network for every subsequent round of every game (the reference's
 * model hot reload with switchNetsMidGame, selfplay.cpp:135-260, play.cpp:1210-1226).
 * On error (unreadable / mismatched model) the current network stays in use. */
int coffee_selfplay_set_model(coffee_selfplay* h, const char* model_path);
/* The same from a CFNN file image in HOST memory (bytes long): a multi-rank host
 * broadcasts the new weights from rank 0 (RCCL) and every rank switches from the
 * received image, instead of each rank re-reading the file. */
int coffee_selfplay_set_model_bytes(coffee_selfplay* h, const void* data, uint64_t bytes);
int coffee_selfplay_destroy(coffee_selfplay* h);

/* ---- two-network match play (replaces the game loop of the reference's gatekeeper,
 *      cpp/command/gatekeeper.cpp:111-187, on the self-play engine's kernels) ----
 * num_games concurrent games between net 0 (the baseline) and net 1 (the candidate).
 * Colour rule: in game number n of global slot s = slot_base + slot the candidate plays
 * black (player 1) iff s + n is even (the reference's {{0,1},{1,0}} pairing).
 * Net choice: every evaluation a game asks for in a round -- root evaluations with their
 * sampled symmetries, leaf evaluations, policy-init opening evaluations -- is done by the
 * net of the ROOT player to move of that game, in that net's own launch (net 0's, then
 * net 1's, on the engine stream), and cached in that net's own evaluation cache.
 * Tree: cleared before every search, so no evaluation of the other net survives a move.
 * Settings that keep a tree or exist only to make training rows are rejected with
 * COFFEE_EINVAL before any device call: cheap_search_prob > 0, reduce_visits != 0, a fork
 * probability > 0, side_position_prob > 0, record_tree_positions != 0, a surprise weight
 * != 0.  init_games_with_policy stays allowed (it gives the openings their variety).
 * As in self-play, a game's moves are chosen without LCB (use_lcb_for_selection is carried
 * in the params and not applied to game moves).
 * Output: finished-game records only; no training rows exist and nothing counts as dropped.
 * The batch cap applies to both nets' rows together, with self-play's round-robin rule;
 * the rounds always run the separate select and backup kernels (COFFEE_FUSED_ROUNDS is
 * ignored). */
typedef struct coffee_match_config {
  int32_t x, y, win_len;
  int32_t num_games;       /* concurrent games on this device (numGameThreads) */
  int32_t node_cap;        /* per-game node pool; 0 = max(2048, 3*max_visits) */
  uint64_t seed;
  int32_t slot_base;       /* global index of slot 0: it enters the colour rule */
  int32_t commit_interval; /* as coffee_selfplay_config */
  int32_t start_stagger;   /* as coffee_selfplay_config */
  const char* model_path[2]; /* CFNN models of net 0 (baseline) and net 1 (candidate), host
                              strings; NULL = the stand-in network (coffee_fake_net) */
  coffee_search_params search; /* coffee_match_params_default */
  int32_t nn_cache_log2;   /* entries of EACH net's evaluation cache = 2^nn_cache_log2; 0 disables */
  int32_t nn_batch_cap;    /* rows per round over both nets' launches together; 0 = the smaller
                              of the two nets' own caps (coffee_selfplay_config.nn_batch_cap) */
  int32_t nn_precision;    /* COFFEE_NN_*: each net resolves it on its own */
  int32_t engines_per_device; /* as coffee_selfplay_config */
} coffee_match_config;

typedef struct coffee_match coffee_match;

typedef struct coffee_match_stats {
  uint64_t rounds;
  uint64_t playouts;
  uint64_t nn_evals[2];       /* network rows evaluated by net 0 / net 1 */
  uint64_t moves;
  uint64_t games_finished;
  uint64_t games_dropped;     /* game records lost to a full record buffer (2 x num_games) */
  uint64_t errors;            /* as coffee_selfplay_stats: nonzero makes stats return COFFEE_EINTERNAL */
  uint64_t nn_precision[2];   /* the precision each net runs (0 = stand-in net) */
  uint64_t nn_batch_peak[2];  /* the largest batch each net was given in one round */
  /* the default precision's running audit (coffee_selfplay_stats), per net: a switch to the
   * accurate instance affects that net, and that net's cache, only */
  uint64_t nn_audits[2];
  uint64_t nn_audit_switches[2];
  double nn_audit_max_diff[2];
} coffee_match_stats;

/* The search values of configs/training/gatekeeper1.cfg (:49, :72-80, :95-106): 150 visits,
 * move temperature 0.5 early / 0.2 with halflife 19, LCB on at 5.0 / 0.15, root FPU
 * reduction 0.1, subtree value bias 0.35; what that config leaves at the reference's
 * defaults: root noise off, root policy temperatures 1, no desired-per-child visits, one
 * root symmetry.  Every play setting off.  Other fields as coffee_search_params_default.
 * That config's useUncertainty (:108-110) is not a field of this struct: uncertainty via
 * coffee_match_set_uncertainty (off unless set). */
void coffee_match_params_default(coffee_search_params* p);
int coffee_match_create(const coffee_match_config* cfg, coffee_match** out);
/* As coffee_selfplay_step / _sync / _stream / _destroy. */
int coffee_match_step(coffee_match* h, int rounds, void* stream);
int coffee_match_sync(coffee_match* h);
int coffee_match_stream(coffee_match* h, void** stream);
int coffee_match_destroy(coffee_match* h);
int coffee_match_stats_get(coffee_match* h, coffee_match_stats* out);
/* As coffee_selfplay_drain_games with header [g][5] i32: (slot, game number, number of
 * moves, winner 0 draw / 1 black / 2 white, the candidate's colour 1 black / 2 white). */
int coffee_match_drain_games(coffee_match* h, int max_games, int32_t* header, uint8_t* moves, int* n_out);
/* Points of n drained games (header [n][5], host): a win 1, a draw 0.5 to each side. */
int coffee_match_score(const int32_t* header, int n, double* candidate_points, double* baseline_points);
/* The self-play inspectors' layouts (coffee_selfplay_game_info / _game_tree / _root_policy). */
int coffee_match_game_info(coffee_match* h, int slot, int64_t* info);
int coffee_match_game_tree(coffee_match* h, int slot, int max_nodes, uint32_t* nodes, uint32_t* edges,
                           int* n_nodes);
int coffee_match_root_policy(coffee_match* h, int slot, float* out);

/* ---- batched position analysis (the engine behind the reference's `katago analysis`,
 *      cpp/command/analysis.cpp, on the self-play engine's round kernels) ----
 * num_slots concurrent searches.  A slot holds one query or is idle; queries wait in a ring in
 * device memory, a finished search is turned into a result on the device and its slot takes
 * the next queued query in the same kernel, so slots never wait for the host.
 * A query is a move list from the empty board (policy positions dir * A + cell, alternating
 * from player 1).  The search is the engine's own: a fresh tree, max_visits root visits.
 * RNG coordinates: the search's stream is seeded from (config seed, stream, game_num) by the
 * formula self-play uses for (seed, global slot, game number), so a result does not depend on
 * the slot that searched it; a nonzero rng_counter sets the stream's position (a self-play
 * game's coffee_selfplay_game_info counter reproduces that game's search of the position).
 * Values are reported as stored: from WHITE's perspective.  The side to move is `pla`.
 * Principal variation of a child: its move, then at every node the child with the most edge
 * visits (ties: lower child slot) until a node without children or a terminal node, at most
 * max_pv_len moves.  (The reference follows play-selection values instead.)
 * Settings that keep a tree or exist only to make rows are rejected with COFFEE_EINVAL before
 * any device call: the list of coffee_match_config plus init_games_with_policy. */
#define COFFEE_ANALYSIS_MAX_MOVES 100
#define COFFEE_ANALYSIS_MAX_PV 16
enum {
  COFFEE_ANALYSIS_OK = 0,            /* searched: the move records are valid */
  COFFEE_ANALYSIS_ILLEGAL_MOVE = 1,  /* info = index of the first illegal move */
  COFFEE_ANALYSIS_GAME_OVER = 2,     /* the move list ends the game: info = winner (0 draw: board full) */
  COFFEE_ANALYSIS_NO_LEGAL_MOVE = 3, /* the side to move has no legal move (a draw) */
  COFFEE_ANALYSIS_NO_ALLOWED_MOVE = 4 /* the query's avoid / allow set leaves no legal move (root restrictions below) */
};

typedef struct coffee_analysis_config {
  int32_t x, y, win_len;
  int32_t num_slots;       /* concurrent searches on this device */
  int32_t node_cap;        /* per-slot node pool; 0 = max(2048, 3*max_visits) */
  uint64_t seed;
  const char* model_path;  /* CFNN model, host string; NULL = the stand-in network */
  coffee_search_params search; /* coffee_analysis_params_default */
  int32_t nn_cache_log2;   /* as coffee_selfplay_config */
  int32_t nn_batch_cap;
  int32_t nn_precision;
  int32_t engines_per_device;
  int32_t commit_interval; /* rounds between report launches; 0 = 8 */
  int32_t query_capacity;  /* >= 1: most queries submitted and not yet drained */
  int32_t max_pv_len;      /* 0..COFFEE_ANALYSIS_MAX_PV */
} coffee_analysis_config;

typedef struct coffee_analysis_query {
  uint64_t id;
  uint64_t rng_counter;    /* 0 = the stream's position after its two game-hash draws */
  uint32_t stream, game_num;
  int32_t num_moves;       /* 0..x*y */
  int32_t max_visits;      /* 0 = search.max_visits; at most node_cap - 4 */
  uint16_t moves[COFFEE_ANALYSIS_MAX_MOVES];
} coffee_analysis_query;

typedef struct coffee_analysis_result {
  uint64_t id;
  int32_t status;          /* COFFEE_ANALYSIS_* */
  int32_t info;
  int32_t turn, pla;       /* of the analysed position (status 1: of the position before the illegal move) */
  uint32_t visits;         /* the root's record, bit copies */
  float weight_sum, utility_avg, win_loss_avg, nn_win, nn_loss;
  int32_t num_children;
  int32_t pad;
} coffee_analysis_result;

typedef struct coffee_analysis_move {  /* one root child, in child-slot order */
  int32_t move;
  uint32_t edge_visits;
  uint32_t visits;         /* the child's record, bit copies */
  float weight_sum, utility_avg, win_loss_avg;
  float prior;             /* the root's NN policy of the move, before temperature and noise */
  float lcb, radius;       /* from the mover's perspective (getSelfUtilityLCBAndRadius) */
  float play_selection_value;
  int32_t order;           /* rank by play-selection value descending, ties by lower child slot */
  int32_t pv_len;
  uint16_t pv[COFFEE_ANALYSIS_MAX_PV];
} coffee_analysis_move;

typedef struct coffee_analysis_stats {
  uint64_t rounds, playouts, nn_evals;
  uint64_t queries_loaded;   /* queries taken from the ring */
  uint64_t queries_finished; /* results written */
  uint64_t queries_rejected; /* of those, answered without a search (status != 0) */
  uint64_t errors;           /* as coffee_selfplay_stats */
  uint64_t nn_precision, nn_audits, nn_audit_switches;
  double nn_audit_max_diff;
} coffee_analysis_stats;

typedef struct coffee_analysis coffee_analysis;

/* coffee_match_params_default with the values of configs/analysis_example.cfg: 500 visits,
 * LCB on at 5.0 / 0.15, one root symmetry; root noise off; chosen_move_subtract and
 * chosen_move_prune 0, so the reported play-selection values are unpruned. */
void coffee_analysis_params_default(coffee_search_params* p);
int coffee_analysis_create(const coffee_analysis_config* cfg, coffee_analysis** out);
/* As coffee_selfplay_step / _sync / _stream / _destroy. */
int coffee_analysis_step(coffee_analysis* h, int rounds, void* stream);
int coffee_analysis_sync(coffee_analysis* h);
int coffee_analysis_stream(coffee_analysis* h, void** stream);
int coffee_analysis_destroy(coffee_analysis* h);
/* Copies up to n queries (host) into the device ring without waiting for the engine stream's
 * work; the slots see them from the next coffee_analysis_step on.  *accepted = how many fit
 * (submitted minus drained never exceeds query_capacity).  A query with num_moves outside 0..x*y, a move >= 4*x*y or max_visits
 * outside 0..node_cap-4 fails the call with COFFEE_EINVAL and submits nothing. */
int coffee_analysis_submit(coffee_analysis* h, const coffee_analysis_query* queries, int n, int* accepted);
/* The checks of coffee_analysis_submit that need only the geometry (no engine, no device). */
int coffee_analysis_query_check(int x, int y, int win_len, const coffee_analysis_query* q);
/* Copies up to max finished results, in completion order, to host arrays: header_out [max],
 * moves_out [max][4*x*y] (records past num_children zeroed; NULL = headers only) and frees
 * their capacity.  Synchronises the engine stream. */
int coffee_analysis_drain(coffee_analysis* h, int max, coffee_analysis_result* header_out,
                          coffee_analysis_move* moves_out, int* n_out);
int coffee_analysis_stats_get(coffee_analysis* h, coffee_analysis_stats* out);
/* The self-play inspectors' layouts (coffee_selfplay_game_info / _game_tree / _root_policy). */
int coffee_analysis_game_info(coffee_analysis* h, int slot, int64_t* info);
int coffee_analysis_game_tree(coffee_analysis* h, int slot, int max_nodes, uint32_t* nodes, uint32_t* edges,
                              int* n_nodes);
int coffee_analysis_root_policy(coffee_analysis* h, int slot, float* out);

/* ---- root move restrictions of analysis (the reference's rootSymmetryPruning,
 *      setup.cpp:639-644, and allowMoves / avoidMoves, analysis.cpp:1030-1097) ----
 * A query's search treats a set of root moves as unavailable, its mask:
 *   root symmetries: s in 0..7 (bit 0 flips y, bit 1 flips x, bit 2 transposes; x != y: 0..3)
 *     under which the packed V1 input of the root position equals the identity's bit for bit;
 *   image of move d*A + c under s: symDir[s][d]*A + symCell[s][c] (coffee_symmetry_move);
 *   avoid set: the query's bits (mode 1), or the complement of its bits (mode 2, allow);
 *   used symmetries: the root symmetries that map the avoid set onto itself (a group);
 *   pruned (root_symmetry_pruning on): a legal, not avoided move with an image under a used
 *     symmetry at a lower position -- the survivor of each orbit is its lowest position;
 *   mask = avoid set + pruned set.
 * The masked moves' entries of the root's noised policy (coffee_analysis_root_policy) are -1,
 * so the root never expands them; noise and temperature are drawn over all legal moves first,
 * so the other entries and the RNG stream are what they are without a mask.  A query whose mask
 * leaves no legal move is answered at once with COFFEE_ANALYSIS_NO_ALLOWED_MOVE. */
typedef struct coffee_analysis_root_options {
  int32_t root_symmetry_pruning; /* 0 */
  int32_t include_policy;        /* 0; 1: coffee_analysis_drain2 fills policy_out */
} coffee_analysis_root_options;
#define COFFEE_ANALYSIS_RESTRICT_WORDS 11
typedef struct coffee_analysis_restrict {  /* one per query, beside it */
  uint32_t avoid[COFFEE_ANALYSIS_RESTRICT_WORDS]; /* bit p of word p / 32: policy position p */
  int32_t mode;                  /* 0 none (bits ignored), 1 avoid the set, 2 allow only the set */
} coffee_analysis_restrict;
typedef struct coffee_analysis_root_info {  /* one per result, beside it */
  uint32_t symmetries;           /* bit s: symmetry s was used (status 0 and 4; else 0) */
  int32_t num_masked;            /* legal root moves in the mask */
} coffee_analysis_root_info;
/* Engine-wide; only before the first submitted query (COFFEE_EINVAL afterwards or for a value
 * other than 0 / 1), like coffee_analysis_set_uncertainty. */
int coffee_analysis_set_root_options(coffee_analysis* h, const coffee_analysis_root_options* opts);
/* coffee_analysis_submit with restrict_in [n] (host; NULL: no query is restricted).  A mode
 * outside 0..2, a set bit at a position >= 4*x*y, or a mode other than 0 on a board with more
 * than 352 positions fails the call with COFFEE_EINVAL and submits nothing. */
int coffee_analysis_submit2(coffee_analysis* h, const coffee_analysis_query* queries,
                            const coffee_analysis_restrict* restrict_in, int n, int* accepted);
/* coffee_analysis_drain that also fills root_out [max] (NULL: skipped) and, on an engine with
 * include_policy, policy_out [max][4*x*y] (NULL: skipped): the root's network policy before
 * temperature, noise and mask, -1 at illegal moves; zeros for a result without a search.
 * policy_out on an engine without include_policy is COFFEE_EINVAL. */
int coffee_analysis_drain2(coffee_analysis* h, int max, coffee_analysis_result* header_out,
                           coffee_analysis_move* moves_out, coffee_analysis_root_info* root_out,
                           float* policy_out, int* n_out);
/* The rule on the host (no engine, no device), the code the kernels run.  colours [x*y] 0 / 1 /
 * 2; hist_cell / hist_dir [n_hist <= 5]: the last moves, most recent first; legal_bits
 * [ceil(4xy/32)] words; avoid_bits [11] words with mode as in coffee_analysis_restrict (mode 0:
 * may be NULL); prune 0 / 1.  mask_out [ceil(4xy/32)] words, *syms_out the used symmetries.
 * Returns the number of legal moves left unmasked (0: the query would be answered with
 * COFFEE_ANALYSIS_NO_ALLOWED_MOVE, or the position has no legal move), or a COFFEE_E* code. */
int coffee_root_mask(int x, int y, int win_len, const uint8_t* colours, const int32_t* hist_cell,
                     const int32_t* hist_dir, int n_hist, const uint32_t* legal_bits, const uint32_t* avoid_bits,
                     int mode, int prune, uint32_t* mask_out, uint32_t* syms_out);
/* The image of policy position `move` under symmetry `sym` (0..7) on an x * y board, or
 * COFFEE_EINVAL. */
int coffee_symmetry_move(int x, int y, int sym, int move);

/* ---- uncertainty weighting of playouts (the reference's useUncertainty) ----
 * An evaluation whose short-term win/loss error the net predicts to be large counts for less
 * in every average above it (Search::computeWeightFromNNOutput, searchupdatehelpers.cpp:98-120):
 *   x   = the row's output [P+3] (the shorttermWinlossError logit)
 *   s   = 0.5 x > 40 ? 0.5 x : log(1 + exp(0.5 x))          (nneval.cpp:789-793)
 *   err = sqrt(s * s * 0.25)
 *   p   = err for exponent 1, sqrt(err) for 0.5, else err ^ exponent
 *   w   = coeff / (p + coeff / max_weight)
 * in f32 with the search's deterministic log / exp / pow.  The node's own evaluation enters its
 * weight_sum, weight_sq_sum and averages with weight w instead of 1, a terminal visit with
 * max_weight.  Off (the default of all three engines), every weight is 1 and nothing changes.
 * The setting is not a coffee_search_params field because that struct keeps its layout. */
typedef struct coffee_uncertainty_params {
  int32_t use_uncertainty;          /* 0 */
  float uncertainty_coeff;          /* 0.25, range [1e-4, 1]  (setup.cpp:546) */
  float uncertainty_exponent;       /* 1.0,  range [0, 2] */
  float uncertainty_max_weight;     /* 8.0,  range [1, 100] */
} coffee_uncertainty_params;
void coffee_uncertainty_params_default(coffee_uncertainty_params* p);
/* The formulas above on the host (no device is touched), bit for bit what the search kernels
 * compute: *err and *weight of one logit (either may be NULL).  With use_uncertainty 0 the
 * weight is 1.  COFFEE_EINVAL for out-of-range or non-finite parameters. */
int coffee_uncertainty_weight(const coffee_uncertainty_params* p, float st_error_logit, float* err, float* weight);
/* Sets the weighting of an engine; in a match one setting serves both nets (gatekeeper1.cfg:
 * 108-110).  Only before the engine's first round, and for analysis before the first query is
 * submitted: a tree never mixes the two rules.  Afterwards, or for out-of-range or non-finite
 * values, COFFEE_EINVAL without touching the device.  With the setting on, word 21 of each
 * coffee_*_game_tree node holds the f32 bits of the node's own evaluation weight (off: 0).
 * A match engine with per-side settings (coffee_match_create2, per_side) refuses the call:
 * its sides carry their own, and word 21 follows the side whose search built the tree. */
int coffee_selfplay_set_uncertainty(coffee_selfplay* h, const coffee_uncertainty_params* p);
int coffee_match_set_uncertainty(coffee_match* h, const coffee_uncertainty_params* p);
int coffee_analysis_set_uncertainty(coffee_analysis* h, const coffee_uncertainty_params* p);

/* ---- variance-scaled exploration and noise pruning (the reference's
 *      cpuctUtilityStdevScale and useNoisePruning, on in its match / analysis / GTP set-ups) ----
 * Stdev factor (getFpuValueForChildrenAssumeVisited, searchexplorehelpers.cpp:256-277): the
 * exploration scaling c * sqrt(total + 0.01) of a node's selection, and of the root's reduced
 * play-selection weight, is multiplied by
 *   factor = 1 + scale * (stdev / prior - 1)
 *   stdev  = prior                                        if visits <= 0 or weight_sum <= 1
 *          = sqrt(max(0, ((u^2 + prior^2) * prior_weight + max(utility_sq_avg, u^2) * weight_sum)
 *                        / (prior_weight + weight_sum - 1) - u^2))        (u = utility_avg)
 * Noise pruning (pruneNoiseWeight, searchupdatehelpers.cpp:423-467): a node's recompute scans
 * its visited children in slot order; a child whose utility lies below the weighted average of
 * the children before it and whose weight exceeds twice its prior's share of their weight loses
 * min(cap, (weight - 2 share) * (1 - exp(-gap / utility_scale))); the node's weight_sum takes
 * the scan's total, and the root's chosen-move subtract / prune amounts are 0.
 * All in f32 with the search's deterministic exp.  Off (scale 0 and pruning 0, the default of
 * all three engines), nothing changes. */
typedef struct coffee_exploration_params {
  int32_t use_noise_pruning;               /* 0 */
  float noise_prune_utility_scale;         /* 0.15, range [0.001, 10] */
  float noise_pruning_cap;                 /* FLT_MAX (1e50 in the reference), finite and >= 0 */
  float cpuct_utility_stdev_prior;         /* 0.40, range [0, 10]; > 0 with scale > 0 */
  float cpuct_utility_stdev_prior_weight;  /* 2.0,  range [0, 100] */
  float cpuct_utility_stdev_scale;         /* 0 (the reference's set-ups: 0.85), range [0, 1] */
} coffee_exploration_params;
void coffee_exploration_params_default(coffee_exploration_params* p);
/* The two formulas on the host (no device is touched), bit for bit what the search kernels
 * compute.  COFFEE_EINVAL for out-of-range or non-finite parameters.
 * _stdev_factor: *factor for a parent with the given statistics.
 * _prune_noise_weight: the scan over n children in order (weight, utility from the parent's side,
 * prior; priors below 1e-30 count as 1e-30): new_weight[n] and *new_total (either may be NULL).
 * The scan runs whatever use_noise_pruning says.  With n <= 1 or a total of the weights <= 1e-5
 * the weights come back unchanged and *new_total is their sum in order. */
int coffee_explore_stdev_factor(const coffee_exploration_params* p, int64_t visits, float weight_sum,
                                float utility_avg, float utility_sq_avg, float* factor);
int coffee_prune_noise_weight(const coffee_exploration_params* p, int n, const float* weight, const float* utility,
                              const float* prior, float* new_weight, float* new_total);
/* Sets both mechanisms of an engine, under coffee_*_set_uncertainty's rules: only before the
 * engine's first round (analysis: before the first query), COFFEE_EINVAL otherwise and for
 * out-of-range or non-finite values, without touching the device.  side: -1 on an engine without
 * per-side settings (one block for both nets), 0 / 1 on a match engine with them
 * (coffee_match_create2, per_side); any other combination is COFFEE_EINVAL. */
int coffee_selfplay_set_exploration(coffee_selfplay* h, const coffee_exploration_params* p);
int coffee_analysis_set_exploration(coffee_analysis* h, const coffee_exploration_params* p);
int coffee_match_set_exploration(coffee_match* h, int side, const coffee_exploration_params* p);
/* Beside coffee_*_game_tree, in its breadth-first node order: priors [max_nodes][P], each node's
 * child priors in slot order (the root's children carry the raw prior; its selection reads
 * coffee_*_root_policy); next_prior / next_pos [max_nodes], each node's cached next expansion
 * (-1 / 0xFFFF: none; unused at the root).  Any output may be NULL. */
int coffee_selfplay_game_tree_priors(coffee_selfplay* h, int slot, int max_nodes, float* priors, float* next_prior,
                                     int32_t* next_pos, int* n_nodes);
int coffee_match_game_tree_priors(coffee_match* h, int slot, int max_nodes, float* priors, float* next_prior,
                                  int32_t* next_pos, int* n_nodes);
int coffee_analysis_game_tree_priors(coffee_analysis* h, int slot, int max_nodes, float* priors, float* next_prior,
                                     int32_t* next_pos, int* n_nodes);

/* ---- wide root noise and futile-visit pruning (the reference's wideRootNoise, on
 *      at 0.04 in its analysis set-up, and futileVisitsThreshold) ----
 * Both act in the root's child selection only, during search only; play-selection values, move
 * choice, LCB, policy targets and the analysis report are untouched.
 * Futile-visit pruning (getExploreSelectionValueOfChild, searchexplorehelpers.cpp:136-147,
 * :193-201), checked before the rootDesiredPerChildVisits funnel: with max_w the largest child
 * weight, wpv = root weight_sum / visits and left = visit limit - root visits,
 *   child:     need = (thr * max_w) * ((edge_visits + 1) / (w + wpv)); futile if child_visits + left < need
 *   new move:  need = (thr * max_w) * (1 / wpv);                       futile if left < need
 * A futile move's selection value is -FLT_MAX (an illegal or masked move's stays -inf).
 * Wide root noise (maybeApplyWideRootNoise, :71-87), on every legal child the funnel did not take
 * and on the best unexpanded move: the prior becomes prior^(1 / (4 wide + 1)) and with probability
 * 1/2 the utility from the mover's side gains wide * |gauss|.  The draws do not come from the
 * game's stream: they are a function of the game's stream seed, the root's turn, the root's
 * visits at the selection and the move's policy position alone.
 * Off (both 0, the default of all three engines), nothing changes. */
typedef struct coffee_root_search_params {
  float wide_root_noise;         /* 0, range [0, 5] */
  float futile_visits_threshold; /* 0, allowed: 0 or [0.01, 1] */
} coffee_root_search_params;
void coffee_root_search_params_default(coffee_root_search_params* p);
/* The two rules on the host (no device is touched), bit for bit what the search kernels compute.
 * COFFEE_EINVAL for out-of-range or non-finite parameters.
 * _wide_root_noise: the smoothed prior and the bonus of the move at policy position pos in the
 * root selection at root_visits visits of turn `turn` of game game_num of global slot
 * global_slot_or_stream (analysis: the query's stream and game number), on an engine created with
 * `seed`.  With wide_root_noise 0: the prior unchanged and bonus 0.  Either output may be NULL.
 * _futile_visits: *futile = 1 if the move is futile (is_new: the unexpanded candidate, whose edge /
 * child arguments are ignored), else 0; always 0 with futile_visits_threshold 0. */
int coffee_wide_root_noise(const coffee_root_search_params* p, uint64_t seed, uint32_t global_slot_or_stream,
                           uint32_t game_num, int32_t turn, uint32_t root_visits, int32_t pos, float prior,
                           float* smoothed_prior, float* bonus);
int coffee_futile_visits(const coffee_root_search_params* p, float max_child_weight, float parent_weight_sum,
                         int64_t parent_visits, int64_t visits_left, int64_t edge_visits, int64_t child_visits,
                         float child_weight, int is_new, int* futile);
/* Sets both rules of an engine, under coffee_*_set_exploration's rules (only before the first
 * round / query; side -1 / 0 / 1 as there). */
int coffee_selfplay_set_root_search(coffee_selfplay* h, const coffee_root_search_params* p);
int coffee_analysis_set_root_search(coffee_analysis* h, const coffee_root_search_params* p);
int coffee_match_set_root_search(coffee_match* h, int side, const coffee_root_search_params* p);

/* ---- parallel playouts per search (the reference's numSearchThreads, 16 per
 *      analysis thread in its analysis set-up, and numVirtualLossesPerThread) ----
 * An analysis engine's setting: latency of one query against throughput of many.  With
 * threads = K a searching slot makes n = min(K, visit limit - root visits) descents a round, one
 * after the other in the order j = 0 .. n-1, and all their leaves go through the network in the
 * round's one batch (descent j of slot g on row g K + j); the backups then run in the same order,
 * and the visit limit is tested once after the last.  A search never overshoots its limit.
 * Virtual losses: every node a descent enters as a child -- its leaf included -- counts one more
 * until that playout's backup.  A child with vl > 0 of them is valued, after the choice between
 * its utility and the first-play urgency and before futile-visit pruning, the
 * rootDesiredPerChildVisits funnel and wide root noise, as
 *   vlw = vl * per_thread;  frac = vlw / (vlw + max(0.25, w));
 *   u = u + (loss - u) * frac;  w = w + vlw        loss: -1 white to move at the parent, +1 black
 * The parent's total child weight, the largest child weight and the new-child candidate do not
 * see them.  Collision: a descent that selects a child still in flight -- a node an earlier
 * descent of the round allocated, not yet evaluated; also through a transposition, which then
 * adds no edge -- is abandoned: its virtual losses come off at once, it counts no visit and
 * takes no row, and the slot makes no further descent that round.  Draws keyed on the root's
 * visits (wide root noise) are the same for the descents of one round.  Every other phase of a
 * slot stays one evaluation a round.  Results are deterministic and independent of the slot
 * count.  threads = 1 (the default) is the engine without the feature, bit for bit. */
#define COFFEE_SEARCH_THREADS_MAX 32
#define COFFEE_ROUND_PATH_MAX 102 /* levels of a path: board area + 2 */
/* leaf_kind of coffee_round_path */
#define COFFEE_LEAF_NN 1        /* a new node, evaluated by the network this round */
#define COFFEE_LEAF_TERMINAL 2  /* a finished game */
#define COFFEE_LEAF_CATCHUP 3   /* an edge with fewer visits than its node (graph search) */
#define COFFEE_LEAF_NOCHILD 4   /* no selectable child: the node's own evaluation again */
#define COFFEE_LEAF_CACHED 6    /* a new node, evaluation taken from the NN cache */
#define COFFEE_LEAF_COLLISION 12
typedef struct coffee_search_threads_info {
  int32_t threads;
  float virtual_losses_per_thread;
  uint64_t descents;            /* descents started so far, abandoned ones included */
  uint64_t collisions;          /* descents abandoned at a collision so far */
  uint64_t live_virtual_losses; /* virtual losses now in the engine's trees (0 between rounds) */
} coffee_search_threads_info;
/* One descent: path_len levels (node, child slot taken there) from the root down; node is the
 * slot's internal node index (equal where two entries name one node; level 0 is the root).  A
 * collision carries one more entry, at [path_len]: the node and the child slot it collided at. */
typedef struct coffee_round_path {
  int32_t leaf_kind, path_len;
  int32_t node[COFFEE_ROUND_PATH_MAX];
  int32_t child_slot[COFFEE_ROUND_PATH_MAX];
} coffee_round_path;
typedef struct coffee_round_paths {
  int32_t num_descents; /* of the slot's last round; 0 when that round was no search round */
  int32_t pad;
  coffee_round_path path[COFFEE_SEARCH_THREADS_MAX];
} coffee_round_paths;
/* threads in 1..COFFEE_SEARCH_THREADS_MAX, virtual_losses_per_thread finite and > 0.  Allowed
 * only while the engine holds no query (every submitted query has its result), COFFEE_EINVAL
 * otherwise.  A round must fit one network launch: COFFEE_EINVAL when num_slots * threads
 * exceeds the batch cap (nn_batch_cap, else the network's own), coffee_last_error() naming both.
 * A refused call leaves the engine as it was.  The arrays are allocated on first use. */
int coffee_analysis_set_search_threads(coffee_analysis* h, int threads, float virtual_losses_per_thread);
int coffee_analysis_search_threads_info(coffee_analysis* h, coffee_search_threads_info* out);
/* The descents of a slot's last round (host output; synchronises the engine stream). */
int coffee_analysis_round_paths(coffee_analysis* h, int slot, coffee_round_paths* out);
/* The valuation above on the host (no device is touched), bit for bit what the kernels compute:
 * mover 1 black / 2 white to move at the parent.  vl = 0 returns utility and weight unchanged. */
int coffee_virtual_loss(float per_thread, uint32_t vl, int mover, float utility, float weight, float* u_out,
                        float* w_out);

/* ---- per-side match settings (the reference's `katago match`, whose search keys
 *      take a bot suffix, cpp/command/match.cpp) ----
 * A match engine whose two sides search with their own parameters and uncertainty weighting,
 * and which may run both sides on one network instance -- the same net with two settings is
 * how a setting's strength is measured.
 * Side: side 1 is what coffee_match_config calls the candidate (black in game n of global slot
 * s iff s + n is even), side 0 the baseline; the game records' candidate colour is side 1's.
 * per_side = 1: every parameter a search reads -- descent, FPU, cpuct, root symmetries, noise
 *   and temperature, uncertainty weight, subtree value bias, graph search, the visit limit and
 *   the move choice at the commit -- is the one of the side that searches.  The game-level
 *   settings stay one per engine and come from cfg->search: init_games_with_policy,
 *   policy_init_area_prop, policy_init_area_temperature (a side that differs there is rejected).
 *   coffee_match_set_uncertainty then returns COFFEE_EINVAL: the sides carry their own.
 *   With node_cap = 0 the default comes from the larger of the two sides' max_visits.
 * per_side = 0: cfg->search and coffee_match_set_uncertainty serve both sides; side[] is ignored.
 * share_net = 1: the two model paths must be equal strings (both NULL counts as equal).  One
 *   network instance, one launch a round on every taken row, one evaluation cache (its payload
 *   is the post-processed policy, the values and the raw short-term error, stored whenever
 *   either side weights by it: an entry serves both sides whichever wrote it, as the
 *   reference shares one NNEvaluator).  coffee_match_stats then reports 0 in
 *   nn_evals[1], nn_batch_peak[1], nn_precision[1] and net 1's audit fields.
 * Rejected with COFFEE_EINVAL before any device call, coffee_last_error() naming the side and
 * the field: a side's parameters that coffee_match_create would reject as cfg->search, a
 * side's uncertainty parameters out of range, a differing game-level field, share_net with
 * unequal model paths, a side's max_visits the node pool cannot serve (node_cap, rounded up
 * to 64, must be >= max_visits + 4). */
typedef struct coffee_match_side {
  coffee_search_params search;
  coffee_uncertainty_params unc;
} coffee_match_side;
typedef struct coffee_match_options {
  int32_t per_side;   /* 0: cfg->search and coffee_match_set_uncertainty serve both sides */
  int32_t share_net;  /* 1: one network instance, one launch per round, one cache */
  coffee_match_side side[2];
} coffee_match_options;
/* opts NULL: coffee_match_create. */
int coffee_match_create2(const coffee_match_config* cfg, const coffee_match_options* opts, coffee_match** out);
/* Elo of a result from one side's view (host, doubles), N = wins + draws + losses:
 *   score  p = (W + D/2) / N
 *   se       = sqrt(((W (1-p)^2 + D (0.5-p)^2 + L p^2) / N) / N)
 *   elo(x)   = -400 log10(1/x - 1)
 *   *elo = elo(p), *elo_lo / *elo_hi = elo(p -/+ 1.96 se), -inf / +inf where the argument
 *   leaves (0, 1)
 *   *los     = 0.5 erfc(-(W - L) / sqrt(2 (W + L))), 0.5 when W + L = 0
 * Any output may be NULL.  COFFEE_EINVAL for a negative count or N = 0. */
int coffee_match_elo(int64_t wins, int64_t draws, int64_t losses, double* score, double* elo, double* elo_lo,
                     double* elo_hi, double* los);

/* ---- start positions (the reference's startPoses, play.cpp:186-248, :400-448) ----
 * A share of the games starts from a sample of a table of positions instead of the empty
 * board.  A sample is a move list from the empty board (policy positions dir * A + cell, black
 * first, 0 <= num_moves < A) with a weight; its unnormalised probability is
 * exp(-num_moves * turn_weight_lambda) * weight (generateCumProbs).  The host turns the
 * probabilities (in double) into 64-bit fixed-point cumulative thresholds: nondecreasing,
 * cum[n-1] = 2^64 - 1, a zero-weight sample repeats its predecessor's threshold and is never
 * picked.  A game's draws, on its own stream after the two game-hash draws and before the
 * policy-init draw: u = uni(); if u < prob, r = next() and the sample is the first i with
 * r < cum[i] (r = 2^64 - 1: the last sample with positive weight).  Without a table or with
 * prob 0 no draw is made and nothing changes.  A game from a sample has the sample's moves as
 * unsearched turns (no rows), mode 4 in its rows' gt[55] (MODE_SGFPOS), gt[53] = its start
 * turn, and its policy-init move count drawn with start_policy_init_area_prop in place of
 * policy_init_area_prop (0: no draw).  The sample's trainingWeight, hint positions and
 * asymmetric playouts of the reference are not built. */
typedef struct coffee_start_position {
  float weight;
  int32_t num_moves;
  uint16_t moves[COFFEE_ANALYSIS_MAX_MOVES];
} coffee_start_position;
typedef struct coffee_start_positions_params {
  float prob;                          /* 0, range [0, 1]     startPosesProb */
  float turn_weight_lambda;            /* 0, range [-10, 10]  startPosesTurnWeightLambda */
  float start_policy_init_area_prop;   /* 0, range [0, 1]     startPosesPolicyInitAreaProp */
} coffee_start_positions_params;
void coffee_start_positions_params_default(coffee_start_positions_params* p);
/* Replays n samples (host) with the device rules at the geometry, one wave per sample:
 * status_out[i] (host) is COFFEE_ANALYSIS_OK, _ILLEGAL_MOVE (info_out[i] = index of the move;
 * also a move >= 4 * x * y, and a num_moves outside 0..A-1 with info -1), _GAME_OVER (info =
 * winner) or _NO_LEGAL_MOVE. */
int coffee_start_positions_check(int x, int y, int win_len, int n, const coffee_start_position* samples,
                                 int32_t* status_out, int32_t* info_out);
/* The thresholds of n samples on the host (no device is touched).  COFFEE_EINVAL for a
 * negative or non-finite weight, a table whose weights are all zero, n < 1 or a lambda
 * outside its range. */
int coffee_start_positions_thresholds(const coffee_start_position* samples, int n, float turn_weight_lambda,
                                      uint64_t* cum_out);
/* The pick alone: the sample of raw draw r under thresholds cum[n] (n >= 1).  This and
 * coffee_start_position_draws below are for a caller that has to verify or reproduce a run:
 * a game's draw r is not an input of coffee_start_position_pick, so the rule at r = 0,
 * r = cum[i] and r = 2^64 - 1, and how many draws a game start consumed, can be observed only
 * through them (like coffee_uncertainty_weight, the kernels' own code on the host). */
int coffee_start_position_index(const uint64_t* cum, int n, uint64_t r, int* index);
/* The sample game game_num of global slot global_slot (slot_base + slot) takes under engine
 * seed `seed`, or -1 for the empty board, on the host with the kernels' own code: the seed
 * formula, the two hash draws, then the draws above.  cum NULL or n 0: no table. */
int coffee_start_position_pick(uint64_t seed, uint32_t global_slot, uint32_t game_num, float prob,
                               const uint64_t* cum, int n, int* index);
/* The same, and the stream's counter after the pick's draws: 2 (the hash draws) when the
 * feature is off, 3 after a u >= prob, 4 after a pick. */
int coffee_start_position_draws(uint64_t seed, uint32_t global_slot, uint32_t game_num, float prob,
                                const uint64_t* cum, int n, int* index, uint64_t* rng_counter);
/* Sets the table of an engine: checks the parameters and every sample (the check kernel above),
 * builds the thresholds and uploads both in order with the engine stream (the call waits for
 * the stream's work, checks on it, then copies).  A bad sample or parameter
 * returns COFFEE_EINVAL (the first bad sample's index in coffee_last_error()) and leaves the
 * engine as it was.  Allowed between steps at any time; applies to every game that starts
 * afterwards; before the engine's first round it also restarts every slot's first game, so
 * those see the table.  n = 0 or prob = 0 turns the feature off. */
int coffee_selfplay_set_start_positions(coffee_selfplay* h, const coffee_start_position* samples, int n,
                                        const coffee_start_positions_params* params);
int coffee_match_set_start_positions(coffee_match* h, const coffee_start_position* samples, int n,
                                     const coffee_start_positions_params* params);
/* Games started from the table so far. */
int coffee_selfplay_start_position_games(coffee_selfplay* h, uint64_t* games);
int coffee_match_start_position_games(coffee_match* h, uint64_t* games);

/* Writes n rows (HOST arrays, drain_rows layout) as a training .npz in the reference's
 * format (TrainingWriteBuffers::writeToZipFile trainingwrite.cpp:566-587): members
 * binaryInputNCHWPacked, globalInputNC, policyTargetsNCMove, globalTargetsNC,
 * valueTargetsNCHW, each a v1.0 .npy with a 256-byte header; written to path.tmp
 * and renamed into place. */
int coffee_write_npz(const char* path, int n, int x, int y, const uint8_t* bin, const float* glob,
                     const int16_t* pol, const float* gtgt, const int8_t* value);

/* Device-side inspection for parity tests and tools (host outputs). */
/* info[16] i64: phase, rootK, nodeCount, rootIdx, gameNum, turn, pla, finished, winner,
 *               playouts, nnEvals, moves, gamesFinished, lastCell, lastDir, rng counter */
int coffee_selfplay_game_info(coffee_selfplay* h, int slot, int64_t* info);
/* Canonical tree of one game: nodes in breadth-first order from the root following
 * child slots in order (index-independent).  Per node 16 f32/u32 words, see DESIGN.md. */
int coffee_selfplay_game_tree(coffee_selfplay* h, int slot, int max_nodes, uint32_t* nodes, uint32_t* edges,
                              int* n_nodes);
/* The root's noised policy [P] (after temperature + Dirichlet). */
int coffee_selfplay_root_policy(coffee_selfplay* h, int slot, float* out);

/* Debug: the Student-t(3) CDF table the search uses (2000 f32). */
int coffee_debug_cdf_table(int x, int y, int win_len, float* out /* host */);
/* Debug: the Zobrist tables by cell (host): board [A][3][2], board2 [A][4][2],
 * player [3][2], init [2] (size-X ^ size-Y hashes), game_over [2]. */
int coffee_debug_zobrist(int x, int y, int win_len, uint64_t* board, uint64_t* board2, uint64_t* player,
                         uint64_t* init, uint64_t* game_over);

/* Kernel timing (HIP events on the engine stream) for roofline reporting:
 * which: 0 select, 1 network, 2 backup, 3 commit (+ rows), 4 backup + the next
 * round's select in one kernel (every round not followed by a commit, with the fast
 * fused network or the stand-in; the environment's COFFEE_FUSED_ROUNDS=0 / 1 at
 * creation: never / always).  Summed ms and launch count of the timed launches.  enable = 0 off, N > 0: every N-th launch of each
 * group is bracketed by an event pair (each pair costs a few microseconds of stream
 * gap, so N > 1 keeps a timed run representative of an untimed one). */
int coffee_selfplay_enable_timing(coffee_selfplay* h, int enable);
int coffee_selfplay_kernel_time(coffee_selfplay* h, int which, double* ms, uint64_t* launches);
/* Network evaluations performed by the timed network launches (sum of their batch sizes). */
int coffee_selfplay_timed_nn_evals(coffee_selfplay* h, uint64_t* evals);

#ifdef __cplusplus
}
#endif

#endif /* KATACOFFEE_H */
