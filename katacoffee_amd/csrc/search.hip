// Batched KataGo MCTS for Coffee: one wave (64 lanes) per game, thousands of games
// per launch.  A self-play round is three launches on one stream:
//   kSelect  — root-symmetry evaluation or one PUCT descent per game, leaf encoded
//              straight into the network batch (search.cpp:920-1165);
//   network  — fused residual net (nn.hip) or the stand-in net over the batch;
//   kBackup  — NN post-processing, leaf value and path backup (searchupdatehelpers.cpp);
// and every few rounds kCommit plays the chosen move for the games whose root reached
// maxVisits, reuses the subtree and writes finished games' training rows.
//
// Semantics are the oracle's (oracle/ora_search.cpp), which cites the reference
// lines; each function below names its oracle counterpart.  Every float result
// is reproduced bit-for-bit: reductions over children use waveSum (the treeSum64
// order), sequential sums run on lane 0 in the oracle's order, transcendental
// functions are detmath.h's dlog/dexp/dpow, and the file is compiled with
// -ffp-contract=off and correctly rounded division/sqrt.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "detmath.h"
#include "engine.h"
#include "kc_board.h"
#include "search.h"

namespace kc {

static constexpr int SVB_IDX_MOVE1 = MAX_P + 1;
static constexpr int SVB_IDX_PLA = 2 * (MAX_P + 1);
static constexpr int SVB_IDX_PAT = 2 * (MAX_P + 1) + 3;
static constexpr int BIG = 0x7fffffff;

KC_D int64_t svbQ(float x) { return llrintf(x * 4294967296.0f); }
KC_D float svbF(int64_t v) { return (float)v * (1.0f / 4294967296.0f); }

// Search blocks are a single wave and only that wave touches its game's arrays
// during a launch.  A wave's LDS and vector-memory instructions are performed in
// program order, so lane-to-lane visibility (one lane writes, all lanes read)
// needs only a compiler barrier; a __syncthreads() fence would additionally make
// every such step wait for all outstanding global stores to reach L2.
KC_D void waveSync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

#ifdef KC_SEARCH_PROFILE
// Cycle accounting of the search kernels (tools/search_phase.py; profiling build
// only): per-block phase cycles, accumulated in LDS during the kernel and added to
// the block's own slot at exit (no contended atomics inside the timed paths).
//  0 select blocks   1 select total   2 loadGame   3 descend   4 path levels
//  5 selectBest      6 expansion      7 encode
// 10 backup blocks  11 backup total  12 postprocess+order  13 path backup  14 leaf value
// 16 commit blocks  17 commit total  18 move choice+targets  19 tree reuse  20 finishGame
// 21 startGame      22 live nodes kept  23 finished games
// per path level (the profiling build drains the memory counters at each mark, SPROF_WAIT,
// so a wait is charged to its own slot: the levels' loads overlap less than in the product)
// 32 descent: wait for the node's record and first edges   33 issue + wait of the children's records
// 34 descent: selection arithmetic                         35 descent levels
// 36 backup: wait for the level's loads   37 arithmetic (with the t-CDF reads and the next levels' load issue)
// 38 backup: stores                       39 backup levels
constexpr int SPROF_N = 48;
constexpr int SPROF_MAXG = 16384;
__device__ unsigned long long g_searchProf[SPROF_MAXG * SPROF_N];
// NN-cache probe: every evaluated leaf's state key goes into an open-addressing set;
// a key already present counts as a potential cross-game cache hit (slot 9).
__device__ unsigned long long* g_probeKeys = nullptr;
__device__ unsigned long long g_probeMask = 0;
KC_D void probeLeafKey(uint64_t k0, uint64_t k1) {
  if(!g_probeKeys)
    return;
  uint64_t key = (k0 ^ (k1 * 0x9e3779b97f4a7c15ULL)) | 1ull;
  uint64_t i = (key >> 7) & g_probeMask;
  for(int probe = 0; probe < 64; probe++, i = (i + 1) & g_probeMask) {
    const unsigned long long prev = atomicCAS(&g_probeKeys[i], 0ull, (unsigned long long)key);
    if(prev == 0ull)
      return;
    if(prev == key) {
      atomicAdd(&g_searchProf[9], 1ull);
      return;
    }
  }
}
KC_D unsigned long long* sprofLds() {
  __shared__ unsigned long long c[SPROF_N];
  return c;
}
#define SPROF_NOW() clock64()
#define SPROF_WAIT() __builtin_amdgcn_s_waitcnt(0)
#define SPROF_INIT()                   \
  do {                                 \
    if(laneId() < SPROF_N)             \
      sprofLds()[laneId()] = 0;        \
    __syncthreads();                   \
  } while(0)
#define SPROF_ADD(i, v)                                 \
  do {                                                  \
    if(laneId() == 0)                                   \
      sprofLds()[(i)] += (unsigned long long)(v);       \
  } while(0)
#define SPROF_FLUSH()                                                           \
  do {                                                                          \
    __syncthreads();                                                            \
    if(blockIdx.x < SPROF_MAXG && (laneId() < 24 || (laneId() >= 32 && laneId() < 40))) \
      g_searchProf[blockIdx.x * SPROF_N + laneId()] += sprofLds()[laneId()];    \
  } while(0)
// per-block maximum of a value over launches (slots 24..31; no contention)
#define SPROF_MAX(i, v)                                                                   \
  do {                                                                                    \
    if(laneId() == 0 && blockIdx.x < SPROF_MAXG) {                                        \
      unsigned long long* q_ = &g_searchProf[blockIdx.x * SPROF_N + (i)];                 \
      const unsigned long long v_ = (unsigned long long)(v);                              \
      if(v_ > *q_)                                                                        \
        *q_ = v_;                                                                         \
    }                                                                                     \
  } while(0)
#else
#define SPROF_NOW() 0ull
#define SPROF_WAIT() \
  do {               \
  } while(0)
#define SPROF_INIT() \
  do {               \
  } while(0)
#define SPROF_ADD(i, v) \
  do {                  \
  } while(0)
#define SPROF_MAX(i, v) \
  do {                  \
  } while(0)
#define SPROF_FLUSH() \
  do {                \
  } while(0)
#endif

// A node's child slots: 0..INLINE_EDGES-1 stored with the node, the rest in its block
// of the game's edge pool (search.h).
struct NodeEdges {
  Edge* inl;
  Edge* pool;  // slot INLINE_EDGES of the node's pool block
  KC_D Edge& operator[](int i) const { return i < INLINE_EDGES ? inl[i] : pool[i - INLINE_EDGES]; }
};

// Per-game view of the SoA arrays.
struct GV {
  const SearchDev& d;
  const DTables& T;
  int g, lane;
  const SP* sp;  // this move's search parameters (moveParams after loadGame)
  const Unc* unc;  // and its uncertainty weighting (match play: the searching side's, bindGame)
  mutable int esel = 0;  // the game's current edge-pool buffer (GameDev::edgeSel; setEdgeSel)
  // the playout's network row and path arrays: the game's own, or descent j's of a wide round
  // (setDescent)
  int row;
  int32_t* wpn = nullptr;
  int32_t* wps = nullptr;
  KC_D GV(const SearchDev& d_, int g_) : d(d_), T(*d_.T), g(g_), lane(laneId()), sp(&d_.sp), unc(&d_.unc), row(g_) {}
  // tables through a readonly noalias kernel argument: uniform reads become scalar loads
  KC_D GV(const SearchDev& d_, const DTables& t_, int g_)
      : d(d_), T(t_), g(g_), lane(laneId()), sp(&d_.sp), unc(&d_.unc), row(g_) {}
  KC_D void setDescent(int j) {
    row = g * d.wideK + j;
    wpn = d.widePathNode + (size_t)row * MAX_DEPTH;
    wps = d.widePathSlot + (size_t)row * MAX_DEPTH;
  }
  KC_D Node* nodes() const { return d.nodes + (size_t)g * d.cap; }
  KC_D Edge* inlineEdges(int n) const { return d.edges + ((size_t)g * d.cap + n) * INLINE_EDGES; }
  KC_D Edge* edgePool() const { return d.edgePool + ((size_t)g * 2 + esel) * d.edgePoolCap; }
  KC_D void setEdgeSel(int sel) const { esel = __builtin_amdgcn_readfirstlane(sel); }
  // child slots of node n whose pool block starts at ebase (Node::edgeBase)
  KC_D NodeEdges edges(int n, uint32_t ebase) const { return NodeEdges{inlineEdges(n), edgePool() + ebase}; }
  KC_D NodeEdges edges(int n) const { return edges(n, nodes()[n].edgeBase); }
  KC_D uint64_t* nodeKey(int n) const { return d.nodeKey + ((size_t)g * d.cap + n) * 2; }
  KC_D float* pol(int n) const { return d.policy + ((size_t)g * d.cap + n) * d.P; }
  KC_D uint32_t* freeList() const { return d.freeList + (size_t)g * d.cap; }
  KC_D uint32_t* allocBits() const { return d.allocBits + (size_t)g * (d.cap / 32); }
  KC_D uint64_t* ttKey() const { return d.ttKey + (size_t)g * d.ttCap * 2; }
  KC_D int32_t* ttNode() const { return d.ttNode + (size_t)g * d.ttCap; }
  KC_D size_t svbBase(int sel) const { return ((size_t)g * 2 + sel) * d.svbCap; }
  KC_D float* accPolicy() const { return d.accPolicy + (size_t)g * d.P; }
  KC_D float* rawPolicy() const { return d.rawPolicy + (size_t)g * d.P; }
  KC_D float* rootNoised() const { return d.rootNoised + (size_t)g * d.P; }
  KC_D int32_t* pathNode() const { return wpn ? wpn : d.pathNode + (size_t)g * MAX_DEPTH; }
  KC_D int32_t* pathSlot() const { return wps ? wps : d.pathSlot + (size_t)g * MAX_DEPTH; }
  KC_D TurnRec* turns() const { return d.turns + (size_t)g * d.maxTurns; }
  KC_D int16_t* turnPol(int t) const { return d.turnPol + ((size_t)g * d.maxTurns + t) * d.P; }
};

// The game's uniform state lives in LDS for the kernel's duration (one wave per
// block): every lane executes the same updates, so same-value LDS writes from
// all lanes are benign and program order keeps them visible to later reads.
// Keeping it out of registers roughly halves the kernels' VGPR use.
static_assert(sizeof(GameDev) % 4 == 0, "GameDev copy granularity");
KC_D void storeGame(const GV& v, const GameDev& s) {
  waveSync();
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&s);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&v.d.games[v.g]);
  for(int i = v.lane; i < (int)(sizeof(GameDev) / 4); i += 64)
    dst[i] = src[i];
}

// Match play: the side (0 / 1) that searches a game's current root, or has just searched it
// (the root and the game number change only in kCommit and in a policy-initialisation backup).
KC_D int sideOf(const SearchDev& d, int g, const GameDev& s) {
  return matchNet(d.slotBase + g, s.gameNum, s.root.pla);
}

// The view's per-game settings from the loaded state.
// MATCH with per-side settings: side 1's searches read sp1 / unc1 (match play
// admits no cheap searches, so a side has one parameter set).
template <bool MATCH = false>
KC_D void bindGame(GV& v, const GameDev& s) {
  // a cheap search without recorded rows runs without root noise and root-specific
  // settings (runBotWithLimits play.cpp:1024-1037); the flag is uniform
  v.sp = __builtin_amdgcn_readfirstlane(s.noNoise) ? &v.d.spCheap : &v.d.sp;
  if constexpr(MATCH) {
    if(v.d.matchPerSide && __builtin_amdgcn_readfirstlane(sideOf(v.d, v.g, s))) {
      v.sp = &v.d.sp1;
      v.unc = &v.d.unc1;
    }
  }
  v.setEdgeSel(s.edgeSel);
}

// The exploration block (explore.h) of the view's side: beside unc / unc1.
KC_D const Expl& explOf(const GV& v) { return v.unc == &v.d.unc1 ? v.d.ex1 : v.d.ex; }
// Likewise the root-search block (rootsearch.h).
KC_D const RootSearch& rootSearchOf(const GV& v) { return v.unc == &v.d.unc1 ? v.d.rs1 : v.d.rs; }

// MATCH with per-side settings: the visit limit of the search about to start is the next
// mover's (setMoveLimits gave side 0's; match play has no cheap or reduced searches).
template <bool MATCH>
KC_D void matchMoveLimits(const GV& v, GameDev& s) {
  if constexpr(MATCH) {
    if(v.d.matchPerSide && __builtin_amdgcn_readfirstlane(sideOf(v.d, v.g, s)))
      s.visitLimit = v.d.sp1.maxVisits;
  }
}

template <bool MATCH = false>
KC_D void loadGame(GV& v, GameDev& s) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&v.d.games[v.g]);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&s);
  for(int i = v.lane; i < (int)(sizeof(GameDev) / 4); i += 64)
    dst[i] = src[i];
  waveSync();
  bindGame<MATCH>(v, s);
}

template <int NI>
KC_D float tsum(const float (&x)[NI], int n, int lane) {
  float a = 0.0f;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = lane + 64 * j;
    if(i < n)
      a = j == 0 ? x[j] : a + x[j];
  }
  return waveSum(a);
}

KC_D int bcastI(int v, int srcLane) { return bcastLane(v, srcLane); }

// Child slots read speculatively with their node record (2 x 128-B lines of Edge).
constexpr int SPEC_EDGES = INLINE_EDGES;
// The board functions' one-word form (kc_board.h) by the kernels' items-per-lane instance:
// laneItems() gives NI <= 4 only to P = 4 A <= 256, that is A <= 64 cells.
template <int NI>
constexpr bool W1_OF = NI <= 4;
KC_D int firstLane(uint64_t m) { return __builtin_ctzll(m); }

KC_D float childWeight(uint32_t edgeVisits, uint32_t childVisits, float rawWeight) {
  return rawWeight * ((float)edgeVisits / (float)(childVisits > 1u ? childVisits : 1u));
}

// ---------------------------------------------------------------------------
// Transposition table (oracle ttFind / ttInsert): linear probing, PROBE_W slots per step.
// The node of key (k0, k1) or -1; on a miss emptySlot is where ttInsert would put it
// (the first free slot of the probe sequence; the table is not changed in between).
// A window's slot and key loads are issued together.  The tables are at most half full,
// so a probe almost always ends in its first few slots: a 16-slot window (lanes 0-15;
// 256 B of keys) instead of the whole wave's 64 (1 KB) keeps the same single round trip
// and cuts the bytes a probe pulls from HBM by 4 (PMC: kSelect read 15 MB per launch).
constexpr int PROBE_W = 16;
KC_D int ttFind(const GV& v, uint64_t k0, uint64_t k1, int& emptySlot) {
  const int mask = v.d.ttCap - 1;
  const int start = (int)(k0 & (uint64_t)mask);
  const uint64_t* key = v.ttKey();
  const int32_t* node = v.ttNode();
  emptySlot = -1;
  const bool act = v.lane < PROBE_W;
  for(int base = 0; base < v.d.ttCap; base += PROBE_W) {
    int s = (start + base + v.lane) & mask;
    const int nd = act ? node[s] : 0;
    const uint64_t ka = act ? key[2 * s] : 0ull, kb = act ? key[2 * s + 1] : 0ull;
    bool match = act && nd >= 0 && ka == k0 && kb == k1;
    uint64_t m = ballot(act && (nd < 0 || match));
    if(m) {
      int f = firstLane(m);
      emptySlot = bcastI(s, f);
      return bcastI(match ? nd : -1, f);
    }
  }
  return -1;
}

KC_D void ttInsertAt(const GV& v, int slot, uint64_t k0, uint64_t k1, int nodeIdx) {
  if(slot >= 0 && v.lane == 0) {
    v.ttKey()[2 * slot] = k0;
    v.ttKey()[2 * slot + 1] = k1;
    v.ttNode()[slot] = nodeIdx;
  }
}

// SVB table (oracle svbFindOrInsert), key 0 = empty.  first: this lane's key of the
// first probe window, loaded ahead by svbProbe (its latency overlaps other work).
KC_D uint64_t svbProbe(const GV& v, int sel, uint64_t k) {
  const int mask = v.d.svbCap - 1;
  return v.lane < PROBE_W ? v.d.svbKey[v.svbBase(sel) + (((int)(k & (uint64_t)mask) + v.lane) & mask)] : 0ull;
}
KC_D int svbFindOrInsert(const GV& v, int sel, uint64_t k, uint64_t first) {
  const int mask = v.d.svbCap - 1;
  const size_t b = v.svbBase(sel);
  const int start = (int)(k & (uint64_t)mask);
  const bool act = v.lane < PROBE_W;
  for(int base = 0; base < v.d.svbCap; base += PROBE_W) {
    int s = (start + base + v.lane) & mask;
    uint64_t kk = base == 0 ? first : (act ? v.d.svbKey[b + s] : 0ull);
    uint64_t m = ballot(act && (kk == 0 || kk == k));
    if(m) {
      int f = firstLane(m);
      int slot = bcastI(s, f);
      bool empty = bcastLane((int)(kk == 0), f) != 0;
      if(empty && v.lane == f) {
        v.d.svbKey[b + slot] = k;
        v.d.svbD[b + slot] = 0;
        v.d.svbW[b + slot] = 0;
      }
      return slot;
    }
  }
  return -1;
}

// SPEC a19 key (oracle svbKey): Zmove0[parentPrev] ^ Zmove1[move] ^ Zpla[mover] ^ 5x5 pattern.
template <bool W1 = false>
KC_D uint64_t svbKeyOf(const GV& v, const DBoard& before, int parentPrevPos, int movePos, int mover) {
  const DTables& T = v.T;
  uint64_t h = 0;
  if(v.lane < 25) {
    int wy = v.lane / 5, wx = v.lane % 5;
    int cell = movePos % T.A;
    int xx = cell % T.X + wx - 2, yy = cell / T.X + wy - 2;
    int col = (xx >= 0 && xx < T.X && yy >= 0 && yy < T.Y) ? colorAt<W1>(before, yy * T.X + xx) : 3;
    h = T.svbZ[SVB_IDX_PAT + col * 25 + wy * 5 + wx];
  }
  h = waveXor64(h);
  h ^= T.svbZ[parentPrevPos] ^ T.svbZ[SVB_IDX_MOVE1 + movePos] ^ T.svbZ[SVB_IDX_PLA + mover];
  return h != 0 ? h : 1;
}

// freeIdx: freeList[freeTop - 1] when the caller loaded it ahead, else -1.
KC_D int allocNode(const GV& v, GameDev& s, int nextPla, uint64_t k0, uint64_t k1, bool terminal, int freeIdx = -1) {
  if(s.freeTop <= 0) {
    s.err = ERR_NODE_POOL;
    return -1;
  }
  s.freeTop--;
  int idx = freeIdx >= 0 ? freeIdx : (int)v.freeList()[s.freeTop];
  if(v.lane == 0) {
    Node n;
    n.visits = 0;
    n.weightSum = n.weightSqSum = n.utilityAvg = n.utilitySqAvg = n.winLossAvg = 0.0f;
    n.nnWin = n.nnLoss = n.lastSvbDelta = n.lastSvbWeight = 0.0f;
    n.svbEntry = -1;
    n.numChildren = 0;
    n.nextPla = (uint8_t)nextPla;
    n.flags = terminal ? 2 : 0;
    n.nextPrior = -1.0f;
    n.nextPos = 0xFFFF;
    n.virtualLosses = 0;
    n.edgeBase = 0;
    n.nnWeight = 1.0f;
    v.nodes()[idx] = n;
    v.nodeKey(idx)[0] = k0;
    v.nodeKey(idx)[1] = k1;
    atomicOr(&v.allocBits()[idx >> 5], 1u << (idx & 31));
  }
  s.liveCount++;
  return idx;
}

// ---------------------------------------------------------------------------
// A node's statistics after an update (what its parent's recompute reads).
struct NStats {
  uint32_t visits;
  float weightSum, weightSqSum, utilityAvg, utilitySqAvg, winLossAvg;
};

// oracle addLeafValue (searchupdatehelpers.cpp:12-82); returns the new statistics.
// weight: the evaluation's weight (uncertainty weighting; 1 with the setting off, and
// x * 1.0f is exact, so the one sequence serves both).
KC_D NStats addLeafValue(const GV& v, const GameDev& s, int ni, float wl, float weight, bool isTerminal,
                         bool assumeNoExisting) {
  const SP& sp = *v.sp;
  Node* np = &v.nodes()[ni];
  const int svbEntry = np->svbEntry;
  uint32_t visits = np->visits;
  float weightSum = np->weightSum, weightSqSum = np->weightSqSum;
  float utilityAvg = np->utilityAvg, utilitySqAvg = np->utilitySqAvg, winLossAvg = np->winLossAvg;
  float utility = wl;
  if(sp.svbFactor != 0.0f && !isTerminal && svbEntry >= 0) {
    size_t e = v.svbBase(s.svbSel) + svbEntry;
    float dd = svbF(v.d.svbD[e]), ww = svbF(v.d.svbW[e]);
    if(ww > 0.001f)
      utility = utility + (sp.svbFactor * dd) / ww;
  }
  float usq = utility * utility;
  if(assumeNoExisting) {
    winLossAvg = wl;
    utilityAvg = utility;
    utilitySqAvg = usq;
    weightSqSum = weight * weight;
    weightSum = weight;
    visits += 1;
  } else {
    float oldW = weightSum, newW = oldW + weight;
    winLossAvg = (winLossAvg * oldW + wl * weight) / newW;
    utilityAvg = (utilityAvg * oldW + utility * weight) / newW;
    utilitySqAvg = (utilitySqAvg * oldW + usq * weight) / newW;
    weightSqSum = weightSqSum + weight * weight;
    weightSum = newW;
    visits += 1;
  }
  waveSync();
  if(v.lane == 0) {
    np->visits = visits;
    np->weightSum = weightSum;
    np->weightSqSum = weightSqSum;
    np->utilityAvg = utilityAvg;
    np->utilitySqAvg = utilitySqAvg;
    np->winLossAvg = winLossAvg;
  }
  waveSync();
  return NStats{visits, weightSum, weightSqSum, utilityAvg, utilitySqAvg, winLossAvg};
}

KC_D float cdfT(const DTables& T, float z) {
  float dd = (1999.0f * (z - (-50.0f))) / 100.0f;
  if(dd <= 0.0f)
    return 0.0f;
  int idx = (int)dd;
  if(idx >= 1999)
    return 1.0f;
  float lambda = dd - (float)idx;
  float y0 = T.cdf[idx], y1 = T.cdf[idx + 1];
  return y0 + lambda * (y1 - y0);
}

// oracle recompute (recomputeNodeStats searchupdatehelpers.cpp:151-328 +
// downweightBadChildrenAndNormalizeWeight :330-419) for one path level, after the path
// edge `slot` gained a visit (the oracle's EV(pn, slot) += 1).  Split in three so the
// backup can run the levels as a pipeline: loadLevel (the node record and its first 64
// edges), loadKids (child records, remaining edges, the node's SVB sums), computeLevel
// (arithmetic and stores).  A level's loads are issued while the level below it is
// computed, so the path child's record and (when the two levels share an SVB entry)
// the SVB sums can be stale: computeLevel takes both from the level below (`below`),
// which is exactly what the sequential order would read.
// (EXPL, the kernels' exploration flag -- DESIGN.md 8g: the noise-pruning scan needs each
// child's prior, which only those instantiations carry)
template <int NI, bool EXPL>
struct PathPriors {};
template <int NI>
struct PathPriors<NI, true> {
  float epr[NI];  // the parent's prior of the child's move (root: the noised root policy)
};
template <int NI, bool EXPL = false>
struct PathLevel : PathPriors<NI, EXPL> {
  int ni, slot, k, nextPla, svbEntry;
  uint32_t ebase;
  float nnWin, nnLoss, nnWeight, lastSvbDelta, lastSvbWeight;
  uint32_t visits0;
  uint32_t ech[NI], evis[NI];  // edge child and visits
  uint32_t cv[NI];
  float cws[NI], cwsq[NI], cu[NI], cusq[NI], cwl[NI];
  int64_t svbD0, svbW0;
};
// What a computed level hands to the level above it.
struct LevelOut {
  NStats st;
  int svbEntry;  // -1: the SVB sums were not written
  int64_t svbD, svbW;
};

template <int NI, bool EXPL>
KC_D void loadLevel(const GV& v, int ni, int slot, PathLevel<NI, EXPL>& L) {
  const Node nd = v.nodes()[ni];
  const Edge* E = v.inlineEdges(ni);
  // the first SPEC_EDGES slots speculatively with the record (slots past numChildren
  // are ignored); the rest once the record says how many there are
  const Edge e0 = v.lane < SPEC_EDGES && v.lane < v.d.P ? E[v.lane] : Edge{0u, 0u, 0.0f, 0u};
  L.ebase = nd.edgeBase;
  L.ech[0] = e0.child;
  L.evis[0] = e0.visits;
  L.ni = ni;
  L.slot = slot;
  L.k = nd.numChildren;
  L.nextPla = nd.nextPla;
  L.svbEntry = nd.svbEntry;
  L.nnWin = nd.nnWin;
  L.nnLoss = nd.nnLoss;
  L.nnWeight = nd.nnWeight;
  L.lastSvbDelta = nd.lastSvbDelta;
  L.lastSvbWeight = nd.lastSvbWeight;
  L.visits0 = nd.visits;
}

template <int NI, bool EXPL>
KC_D void loadKids(const GV& v, const GameDev& s, PathLevel<NI, EXPL>& L) {
  const SP& sp = *v.sp;
  const NodeEdges E = v.edges(L.ni, L.ebase);
  const Node* NS = v.nodes();
#pragma unroll
  for(int j = 0; j < NI; j++) {
    const int i = v.lane + 64 * j;
    L.cv[j] = 0;
    L.cws[j] = L.cwsq[j] = L.cu[j] = L.cusq[j] = L.cwl[j] = 0.0f;
    if constexpr(EXPL)
      L.epr[j] = 0.0f;
    if(j > 0 || i >= SPEC_EDGES)
      L.ech[j] = L.evis[j] = 0u;
    if(i < L.k) {
      if(j > 0 || i >= SPEC_EDGES) {
        const Edge e = E[i];
        L.ech[j] = e.child;
        L.evis[j] = e.visits;
      }
      if constexpr(EXPL) {
        // the edge again for its prior and move (the speculative read kept neither)
        const Edge e = E[i];
        L.epr[j] = L.ni == s.rootIdx ? v.rootNoised()[e.move] : e.prior;
      }
      const Node& c = NS[L.ech[j]];
      L.cv[j] = c.visits;
      L.cws[j] = c.weightSum;
      L.cwsq[j] = c.weightSqSum;
      L.cu[j] = c.utilityAvg;
      L.cusq[j] = c.utilitySqAvg;
      L.cwl[j] = c.winLossAvg;
    }
  }
  // unconditional (entry 0 when the node has none; ignored then): no branch between
  // the pipeline's loads and the waits on them
  const size_t e = v.svbBase(s.svbSel) + (L.svbEntry >= 0 ? L.svbEntry : 0);
  L.svbD0 = v.d.svbD[e];
  L.svbW0 = v.d.svbW[e];
  (void)sp;
}

// issueNext() issues the next levels' loads; it runs right after this level's t-CDF
// table reads, the last loads the level waits on (vmcnt counts in issue order, so a
// wait on a load also waits on every older one).
template <int NI, bool EXPL, class F>
KC_D LevelOut computeLevel(const GV& v, const GameDev& s, PathLevel<NI, EXPL>& L, const LevelOut& below, bool haveBelow,
                           int numVisitsToAdd, bool isRoot, F&& issueNext) {
  const SP& sp = *v.sp;
  const unsigned long long tLoads = SPROF_NOW();
  (void)tLoads;
  SPROF_WAIT();
  const unsigned long long tCalc = SPROF_NOW();
  (void)tCalc;
  SPROF_ADD(36, tCalc - tLoads);
  SPROF_ADD(39, 1);
  const int k = L.k, slot = L.slot;
  const int nextPla = L.nextPla;
  const int svbEntry = L.svbEntry;
  const NodeEdges E = v.edges(L.ni, L.ebase);
  const bool svbOn = sp.svbFactor != 0.0f && svbEntry >= 0;
  int64_t svbD0 = L.svbD0, svbW0 = L.svbW0;
  if(svbOn && haveBelow && below.svbEntry == svbEntry) {
    svbD0 = below.svbD;
    svbW0 = below.svbW;
  }
  bool good[NI];
  float wAdj[NI], selfU[NI], cU[NI], cUsq[NI], cWl[NI], cWs[NI], cWsq[NI], tmp[NI];
  int numGood = 0;
  float maxW = 0.0f;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = v.lane + 64 * j;
    good[j] = false;
    wAdj[j] = selfU[j] = cU[j] = cUsq[j] = cWl[j] = cWs[j] = cWsq[j] = 0.0f;
    if(i < k) {
      uint32_t evis = L.evis[j];
      uint32_t cv = L.cv[j];
      float ws = L.cws[j], wsq = L.cwsq[j], u = L.cu[j], usq = L.cusq[j], wl = L.cwl[j];
      if(i == slot) {
        evis += 1;
        E[i].visits = evis;
        if(haveBelow) {
          cv = below.st.visits;
          ws = below.st.weightSum;
          wsq = below.st.weightSqSum;
          u = below.st.utilityAvg;
          usq = below.st.utilitySqAvg;
          wl = below.st.winLossAvg;
        }
      }
      good[j] = cv > 0 && ws > 0.0f && evis > 0;
      if(good[j]) {
        cU[j] = u;
        cUsq[j] = usq;
        cWl[j] = wl;
        cWs[j] = ws;
        cWsq[j] = wsq;
        selfU[j] = nextPla == 2 ? cU[j] : -cU[j];
        wAdj[j] = childWeight(evis, cv, ws);
        maxW = wAdj[j] > maxW ? wAdj[j] : maxW;
      }
    }
    numGood += __popcll(ballot(good[j]));
  }
  maxW = waveMax(maxW);
  const float origTotal = tsum<NI>(wAdj, k, v.lane);
  float currentTotal = origTotal;
  bool pruning = false;
  if constexpr(EXPL) {
    // noise pruning (explore.h): the serial scan over the good children in slot order, run by
    // every lane on broadcasts of the slot's values; the slot's own lane keeps the new weight.
    // currentTotal is the scan's own sum.
    const Expl& ex = explOf(v);
    pruning = ex.noisePruning != 0;
    if(pruning && pruneNoiseApplies(numGood, origTotal)) {
      PruneScan sc{0.0f, 0.0f, 0.0f};
#pragma unroll
      for(int j = 0; j < NI; j++) {
        const int cnt = k - 64 * j < 64 ? k - 64 * j : 64;  // uniform
        const uint64_t gm = ballot(good[j]);
        for(int l = 0; l < cnt; l++) {
          if(!((gm >> l) & 1ull))
            continue;
          const float old = bcastLaneF(wAdj[j], l), u = bcastLaneF(selfU[j], l), pr = bcastLaneF(L.epr[j], l);
          const float nw = pruneNoiseStep(ex, sc, old, u, pr);
          if(v.lane == l)
            wAdj[j] = nw;
        }
      }
      currentTotal = sc.wSum;
    }
  }
  float amountToSubtract = 0.0f, amountToPrune = 0.0f;
  if(isRoot && sp.rootNoise && !pruning) {
    amountToSubtract = fminf(sp.moveSubtract, maxW / 64.0f);
    amountToPrune = fminf(sp.movePrune, maxW / 64.0f);
  }
  if(numGood > 0 && currentTotal > 0.0f) {
    float stdev[NI];
#pragma unroll
    for(int j = 0; j < NI; j++) {
      if(j > 0 && 64 * j >= k) {  // uniform: no lane has an item here
        stdev[j] = tmp[j] = 0.0f;
        continue;
      }
      stdev[j] = good[j] ? sqrtf(1e-8f + 1.0f / (1.5f * sqrtf(wAdj[j]))) : 0.0f;
      tmp[j] = good[j] ? selfU[j] * wAdj[j] : 0.0f;
    }
    const float simpleValue = tsum<NI>(tmp, k, v.lane) / currentTotal;
    // cdfT split: the table reads of every item first, then the next levels' loads,
    // then the interpolation (same arithmetic)
    float y0[NI], y1[NI], lam[NI], pc[NI];
    int mode[NI];  // 0 skip, 1 table, 2 constant pc
#pragma unroll
    for(int j = 0; j < NI; j++) {
      mode[j] = 0;
      y0[j] = y1[j] = lam[j] = pc[j] = 0.0f;
      if(j > 0 && 64 * j >= k)
        continue;
      if(!good[j] || wAdj[j] < amountToPrune)
        continue;
      float z = (selfU[j] - simpleValue) / stdev[j];
      float dd = (1999.0f * (z - (-50.0f))) / 100.0f;
      if(dd <= 0.0f) {
        mode[j] = 2;
        pc[j] = 0.0f;
        continue;
      }
      int idx = (int)dd;
      if(idx >= 1999) {
        mode[j] = 2;
        pc[j] = 1.0f;
        continue;
      }
      mode[j] = 1;
      lam[j] = dd - (float)idx;
      y0[j] = v.T.cdf[idx];
      y1[j] = v.T.cdf[idx + 1];
    }
    issueNext();
#pragma unroll
    for(int j = 0; j < NI; j++) {
      if((j > 0 && 64 * j >= k) || mode[j] == 0) {
        tmp[j] = 0.0f;
        continue;
      }
      float nw = wAdj[j] - amountToSubtract;
      if(nw <= 0.0f)
        nw = 0.0f;
      const float c = mode[j] == 1 ? y0[j] + lam[j] * (y1[j] - y0[j]) : pc[j];
      float p = c + 0.0001f;
      float f = sp.valueWeightExp == 0.5f ? sqrtf(p) : dpow(p, sp.valueWeightExp);
      tmp[j] = nw * f;
    }
    const float totalNew = tsum<NI>(tmp, k, v.lane);
    const float factor = currentTotal / totalNew;
#pragma unroll
    for(int j = 0; j < NI; j++)
      wAdj[j] = tmp[j] * factor;
  } else {
    issueNext();
  }
  float wlv[NI], uv[NI], usqv[NI], wsqv[NI];
#pragma unroll
  for(int j = 0; j < NI; j++) {
    if((j > 0 && 64 * j >= k) || !good[j]) {
      wlv[j] = uv[j] = usqv[j] = wsqv[j] = 0.0f;
      continue;
    }
    float ws = wAdj[j] / cWs[j];
    wlv[j] = wAdj[j] * cWl[j];
    uv[j] = wAdj[j] * cU[j];
    usqv[j] = wAdj[j] * cUsq[j];
    wsqv[j] = (ws * ws) * cWsq[j];
  }
  float winLossSum = tsum<NI>(wlv, k, v.lane);
  float utilitySum = tsum<NI>(uv, k, v.lane);
  float utilitySqSum = tsum<NI>(usqv, k, v.lane);
  float weightSqSum = tsum<NI>(wsqv, k, v.lane);
  float weightSum = currentTotal;
  float wl = L.nnWin - L.nnLoss;
  float utility = wl;
  float newLastD = L.lastSvbDelta, newLastW = L.lastSvbWeight;
  LevelOut out;
  out.svbEntry = -1;
  out.svbD = out.svbW = 0;
  if(svbOn) {
    int64_t D = svbD0, Wt = svbW0;
    if(currentTotal > 1e-10f) {
      float utilityChildren = utilitySum / currentTotal;
      float svbWv = dpow(origTotal, sp.svbExp);
      float svbDv = (utilityChildren - utility) * svbWv;
      D += svbQ(svbDv) - svbQ(L.lastSvbDelta);
      Wt += svbQ(svbWv) - svbQ(L.lastSvbWeight);
      waveSync();
      if(v.lane == 0) {
        const size_t e = v.svbBase(s.svbSel) + svbEntry;
        v.d.svbD[e] = D;
        v.d.svbW[e] = Wt;
      }
      newLastD = svbDv;
      newLastW = svbWv;
      out.svbEntry = svbEntry;
      out.svbD = D;
      out.svbW = Wt;
    }
    float dd = svbF(D), ww = svbF(Wt);
    if(ww > 0.001f)
      utility = utility + (sp.svbFactor * dd) / ww;
  }
  // the node's own evaluation at its weight (searchupdatehelpers.cpp:291-300; 1 with
  // uncertainty weighting off)
  const float selfW = L.nnWeight;
  winLossSum = winLossSum + wl * selfW;
  utilitySum = utilitySum + utility * selfW;
  utilitySqSum = utilitySqSum + (utility * utility) * selfW;
  weightSqSum = weightSqSum + selfW * selfW;
  weightSum = weightSum + selfW;
  out.st.winLossAvg = winLossSum / weightSum;
  out.st.utilityAvg = utilitySum / weightSum;
  out.st.utilitySqAvg = utilitySqSum / weightSum;
  out.st.weightSqSum = weightSqSum;
  out.st.weightSum = weightSum;
  out.st.visits = L.visits0 + (uint32_t)numVisitsToAdd;
  waveSync();
  const unsigned long long tStore = SPROF_NOW();
  (void)tStore;
  SPROF_ADD(37, tStore - tCalc);
  if(v.lane == 0) {
    Node* np = &v.nodes()[L.ni];
    np->winLossAvg = out.st.winLossAvg;
    np->utilityAvg = out.st.utilityAvg;
    np->utilitySqAvg = out.st.utilitySqAvg;
    np->weightSqSum = out.st.weightSqSum;
    np->weightSum = out.st.weightSum;
    np->visits = out.st.visits;
    np->lastSvbDelta = newLastD;
    np->lastSvbWeight = newLastW;
  }
  waveSync();
  SPROF_ADD(38, SPROF_NOW() - tStore);
  return out;
}

// The path from the deepest level to the root.  The loads of level j-1 (record and
// first edges, then child records) and the record of level j-2 are issued before
// level j is computed; with more than two items per lane (register budget) the
// levels run one at a time.
template <int NI, bool EXPL = false>
KC_D void backupPath(const GV& v, const GameDev& s, int pathLen, NStats leaf, bool haveLeaf) {
  const int32_t* pn = v.pathNode();
  const int32_t* ps = v.pathSlot();
  // the path in registers (lane j holds level j; levels >= 64 re-read), one load
  const int myNode = v.lane < pathLen ? pn[v.lane] : 0, mySlot = v.lane < pathLen ? ps[v.lane] : 0;
  auto nodeAt = [&](int j) { return j < 64 ? bcastLane(myNode, j) : pn[j]; };
  auto slotAt = [&](int j) { return j < 64 ? bcastLane(mySlot, j) : ps[j]; };
  if(pathLen <= 0)
    return;
  LevelOut below;
  bool haveBelow = haveLeaf;
  below.st = leaf;
  below.svbEntry = -1;
  below.svbD = below.svbW = 0;
  int j = pathLen - 1;
  if constexpr(NI > 2) {
    // wide levels (7x7, 9x9): one level at a time
    for(; j >= 0; j--) {
      PathLevel<NI, EXPL> cur;
      loadLevel<NI, EXPL>(v, nodeAt(j), slotAt(j), cur);
      loadKids<NI, EXPL>(v, s, cur);
      below = computeLevel<NI, EXPL>(v, s, cur, below, haveBelow, 1, cur.ni == s.rootIdx, [] {});
      haveBelow = true;
    }
    return;
  }
  PathLevel<NI, EXPL> cur, nxt;
  loadLevel<NI, EXPL>(v, nodeAt(j), slotAt(j), cur);
  if(j > 0)
    loadLevel<NI, EXPL>(v, nodeAt(j - 1), slotAt(j - 1), nxt);
  loadKids<NI, EXPL>(v, s, cur);
  for(; j >= 0; j--) {
    PathLevel<NI, EXPL> nn;
    // the child records of the level above and the record two levels up, issued
    // while this level is computed
    auto issueNext = [&] {
      if(j > 0)
        loadKids<NI, EXPL>(v, s, nxt);
      if(j > 1)
        loadLevel<NI, EXPL>(v, nodeAt(j - 2), slotAt(j - 2), nn);
    };
    below = computeLevel<NI, EXPL>(v, s, cur, below, haveBelow, 1, cur.ni == s.rootIdx, issueNext);
    haveBelow = true;
    if(j > 0) {
      cur = nxt;
      nxt = nn;
    }
  }
}

// oracle fpuValue (searchexplorehelpers.cpp:245-301)
KC_D float fpuValue(const SP& sp, const Node& n, int pla, bool isRoot, float probMass) {
  float parentUtility = n.utilityAvg;
  float forFpu = parentUtility;
  if(sp.fpuByVisited) {
    float pw = sp.fpuByVisitedPow == 2.0f ? probMass * probMass : dpow(probMass, sp.fpuByVisitedPow);
    float avgWeight = fminf(1.0f, pw);
    forFpu = avgWeight * parentUtility + (1.0f - avgWeight) * (n.nnWin - n.nnLoss);
  }
  float redMax = isRoot ? sp.rootFpuRedMax : sp.fpuRedMax;
  float lossProp = isRoot ? sp.rootFpuLossProp : sp.fpuLossProp;
  float reduction = redMax * sqrtf(probMass);
  float fpu = pla == 2 ? forFpu - reduction : forFpu + reduction;
  float lossValue = pla == 2 ? -1.0f : 1.0f;
  fpu = fpu + (lossValue - fpu) * lossProp;
  return fpu;
}

KC_D float exploreScaling(const SP& sp, float totalChildWeight) {
  float c = sp.cpuct;
  if(sp.cpuctLog != 0.0f)
    c = c + sp.cpuctLog * dlog((totalChildWeight + sp.cpuctBase) / sp.cpuctBase);
  return c * sqrtf(totalChildWeight + 0.01f);
}

// oracle selectBest (selectBestChildToDescend searchexplorehelpers.cpp:304-451)
// Also returns the chosen existing child's edge and the child's visits and flags,
// broadcast from the lane that holds them (no reload of either after the choice).
// (VL, the wide kernels' flag -- DESIGN.md 8j: a child's virtual losses enter its value and weight,
// vloss.h; every other instantiation holds no trace of them)
template <int NI, bool EXPL = false, bool VL = false>
KC_D int selectBest(const GV& v, const GameDev& s, int ni, const Node& n, const float* pol, bool isRoot, int& newPos,
                    uint32_t* hasBits, const Edge& e0, Edge& ce, uint32_t& cVisits, uint32_t& cFlags) {
  const SP& sp = *v.sp;
  const int P = v.d.P;
  const int k = n.numChildren;
  const int pla = n.nextPla;
  if(isRoot) {
    for(int w = v.lane; w < (P + 31) / 32; w += 64)
      hasBits[w] = 0;
    waveSync();
  }
  const unsigned long long tKids = SPROF_NOW();
  (void)tKids;
  const NodeEdges E = v.edges(ni, n.edgeBase);
  const Node* NS = v.nodes();
  float probs[NI], cw[NI], pv[NI], cu[NI];
  uint32_t cvis[NI], cfl[NI];
  [[maybe_unused]] uint32_t cvl[NI];
  Edge ev[NI];
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = v.lane + 64 * j;
    probs[j] = cw[j] = pv[j] = cu[j] = 0.0f;
    cvis[j] = cfl[j] = 0;
    if constexpr(VL)
      cvl[j] = 0;
    ev[j] = Edge{0u, 0u, 0.0f, 0u};
    if(j > 0 && 64 * j >= k)  // uniform: no lane has an item here
      continue;
    if(i < k) {
      const Edge e = j == 0 && i < SPEC_EDGES ? e0 : E[i];
      ev[j] = e;
      const Node& c = NS[e.child];
      float p = isRoot ? pol[e.move] : e.prior;
      cvis[j] = c.visits;
      cfl[j] = c.flags;
      if constexpr(VL)
        cvl[j] = c.virtualLosses;
      cu[j] = c.utilityAvg;
      pv[j] = p;
      probs[j] = p < 0.0f ? 0.0f : p;
      cw[j] = p < 0.0f ? 0.0f : childWeight(e.visits, cvis[j], c.weightSum);
      if(isRoot)
        atomicOr(&hasBits[e.move >> 5], 1u << (e.move & 31));
    }
  }
  SPROF_WAIT();
  const unsigned long long tArith = SPROF_NOW();
  (void)tArith;
  SPROF_ADD(33, tArith - tKids);
  const float probMass = tsum<NI>(probs, k, v.lane);
  const float total = tsum<NI>(cw, k, v.lane);
  const float fpu = fpuValue(sp, n, pla, isRoot, probMass);
  float scaling = exploreScaling(sp, total);
  if constexpr(EXPL)
    scaling = scaling * exploreStdevFactor(explOf(v), n.visits, n.weightSum, n.utilityAvg, n.utilitySqAvg);
  // wide root noise and futile-visit pruning (rootsearch.h): the root only, behind
  // wave-uniform tests.  The draws are each move's own (wideRootKey, its policy position).
  float rsWide = 0.0f, rsThr = 0.0f, rsMaxW = 0.0f, rsWpv = 0.0f, rsLeft = 0.0f;
  uint64_t rsKey = 0;
  if constexpr(EXPL) {
    if(isRoot) {
      const RootSearch& rs = rootSearchOf(v);
      rsWide = rs.wide;
      rsThr = rs.thr;
      if(rsWide > 0.0f)
        rsKey = wideRootKey(s.rngSeed, s.root.turn, n.visits);
      if(rsThr > 0.0f) {
        // (masked children carry weight 0 and weights are never negative)
        float m = 0.0f;
#pragma unroll
        for(int j = 0; j < NI; j++)
          m = fmaxf(m, cw[j]);
        rsMaxW = waveMax(m);
        rsWpv = n.weightSum / (float)n.visits;
        rsLeft = (float)(s.visitLimit - (int32_t)n.visits);
      }
    }
  }
  float best = -__builtin_inff();
  int bestIdx = BIG;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = v.lane + 64 * j;
    if((j > 0 && 64 * j >= k) || i >= k)
      continue;
    float p = pv[j];
    float val;
    if(p < 0.0f)
      val = -__builtin_inff();
    else {
      float w = cw[j];
      float u = (cvis[j] == 0 || w <= 0.0f) ? fpu : cu[j];
      if constexpr(VL)
        virtualLossAdjust(v.d.vlPerThread, cvl[j], pla, u, w);
      bool futile = false;
      if constexpr(EXPL)
        futile = rsThr > 0.0f && futileChild(rsThr, rsMaxW, rsWpv, rsLeft, ev[j].visits, cvis[j], w);
      if(futile)
        val = FUTILE_VALUE;
      else if(isRoot && sp.rootDesiredCoeff > 0.0f && p > 0.0f && w < sqrtf((p * total) * sp.rootDesiredCoeff))
        val = 1e20f;
      else {
        if constexpr(EXPL) {
          if(rsWide > 0.0f) {
            u = wideUtility(u, wideBonus(rsWide, rsKey, (int)ev[j].move), pla);
            p = wideSmoothedPrior(rsWide, p);
          }
        }
        val = (scaling * p) / (1.0f + w) + (pla == 2 ? u : -u);
      }
    }
    if(val > best) {
      best = val;
      bestIdx = i;
    }
  }
  waveArgmax(best, bestIdx);
  int bestSlot = best > -__builtin_inff() ? bestIdx : -1;
  if(bestSlot >= 0) {
    Edge me{0u, 0u, 0.0f, 0u};
    uint32_t mv = 0, mf = 0;
#pragma unroll
    for(int j = 0; j < NI; j++)
      if(j == (bestSlot >> 6)) {
        me = ev[j];
        mv = cvis[j];
        mf = cfl[j];
      }
    const int bl = bestSlot & 63;
    ce.child = (uint32_t)bcastLane((int)me.child, bl);
    ce.visits = (uint32_t)bcastLane((int)me.visits, bl);
    ce.move = (uint32_t)bcastLane((int)me.move, bl);
    ce.prior = 0.0f;
    cVisits = (uint32_t)bcastLane((int)mv, bl);
    cFlags = (uint32_t)bcastLane((int)mf, bl);
  }
  float bp = -1.0f;
  int bpos = BIG;
  if(isRoot) {
    // root priors carry noise: scan every unexpanded legal move
    waveSync();
    for(int pos = v.lane; pos < P; pos += 64) {
      if((hasBits[pos >> 5] >> (pos & 31)) & 1u)
        continue;
      float p = pol[pos];
      if(p < 0.0f)
        continue;
      if(p > bp) {
        bp = p;
        bpos = pos;
      }
    }
    waveArgmax(bp, bpos);
  } else if(n.nextPos != 0xFFFF) {
    // non-root: children are always created in prior order, so the best
    // unexpanded move is the k-th entry of the node's expansion order, which
    // the node record caches
    bp = n.nextPrior;
    bpos = n.nextPos;
  }
  newPos = -1;
  if(bpos != BIG) {
    float val;
    bool futile = false;
    if constexpr(EXPL)
      futile = rsThr > 0.0f && futileNew(rsThr, rsMaxW, rsWpv, rsLeft);
    if(futile)
      val = FUTILE_VALUE;
    else {
      float u = fpu;
      if constexpr(EXPL) {
        // (the candidate stays the move of the largest raw prior; one draw, every lane the same)
        if(rsWide > 0.0f) {
          u = wideUtility(u, wideBonus(rsWide, rsKey, bpos), pla);
          bp = wideSmoothedPrior(rsWide, bp);
        }
      }
      val = (scaling * bp) / 1.0f + (pla == 2 ? u : -u);
    }
    if(val > best) {
      bestSlot = k;
      newPos = bpos;
    }
  }
  SPROF_ADD(34, SPROF_NOW() - tArith);
  return bestSlot;
}

// A non-root node's expansion order is its legal moves by descending prior, ties by
// ascending position -- the order selectBest's new-child scan yields
// (selectBestChildToDescend searchexplorehelpers.cpp:304-451: "first strictly
// greater" over positions).  The node caches only its next entry (Node::nextPrior /
// nextPos); the entry after (curPrior, curPos) is found when that one is expanded by
// one scan of the node's policy: the highest prior below curPrior, or equal to it at a
// higher position.  pv: the node's policy, lane-strided (illegal = -1).  No entry:
// (-1, 0xFFFF).
template <int NI>
KC_D void nextExpansion(const GV& v, const float (&pv)[NI], float curPrior, int curPos, float& nPrior, int& nPos) {
  const int P = v.d.P;
  float best = -1.0f;
  int bi = BIG;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    const int p = v.lane + 64 * j;
    const float x = pv[j];
    if(p < P && x >= 0.0f && (x < curPrior || (x == curPrior && p > curPos)) && x > best) {
      best = x;
      bi = p;
    }
  }
  waveArgmax(best, bi);
  nPrior = bi != BIG ? best : -1.0f;
  nPos = bi != BIG ? bi : 0xFFFF;
}

// Parallel playouts: a node entered as a child carries one more virtual loss until
// the playout's backup (or its collision) takes it off again.  Lane 0 alone writes the count.
// (The barrier keeps lane 0's branch apart from the all-lane updates of the game's LDS copy
// before it: merged into one divergent region, lane 0 would run those a second time.)
KC_D void addVirtualLoss(const GV& v, int node) {
  waveSync();
  if(v.lane == 0)
    v.nodes()[node].virtualLosses += 1;
}
// The virtual losses of a playout whose path holds pathLen levels and ends at node `last` come
// off: it entered the path's nodes below the root and `last` (nothing when it never left the
// root).  The nodes of a path are distinct, so each lane takes one.
KC_D void removeVirtualLosses(const GV& v, int pathLen, int last) {
  waveSync();
  const int32_t* pn = v.pathNode();
  for(int i = v.lane; i < pathLen; i += 64)
    v.nodes()[i + 1 < pathLen ? pn[i + 1] : last].virtualLosses -= 1;
  waveSync();
}

// One more level on the playout's path.  The game's LDS copy is updated by all lanes at once,
// each writing the same value.  The VL instantiations follow the update with a lane-0 branch
// (addVirtualLoss): there every lane takes the new length into a register first and writes it
// between barriers, so a lane that ran the update apart from the others would still write the
// same value -- the result does not depend on where the compiler places the code.
template <bool VL>
KC_D void pushLevel(GameDev& s) {
  if constexpr(VL) {
    const int len = s.pathLen + 1;
    waveSync();
    s.pathLen = len;
    waveSync();
  } else {
    s.pathLen++;
  }
}

// oracle descend (playoutDescend search.cpp:936-1165, allocateOrFindNode :704-759,
// maybeCatchUpEdgeVisits :1169-1207)
// VL (the wide kernels): one of a round's several descents.  The selections see the
// virtual losses of the descents before it, every node it enters gains one, and a child still
// in flight -- allocated by an earlier descent of the round, not evaluated yet -- ends it as
// LEAF_COLLISION at the parent, nothing linked or entered there.  loadRootPol: the root's noised
// policy is not in rootPol yet (the round's first descent).
template <int NI, bool EXPL = false, bool VL = false>
KC_D void descend(const GV& v, GameDev& s, uint32_t* hasBits, float* rootPol /* LDS [P] */, bool loadRootPol = true) {
  constexpr bool W1 = W1_OF<NI>;
  const SP& sp = *v.sp;
  const DTables& T = v.T;
  s.pathLen = 0;
  DBoard b = s.root;
  int ni = s.rootIdx;
  uint32_t scanned = 0;  // children of the path nodes (tree-roofline accounting)
  // the first SPEC_EDGES child slots (two cache lines) are read speculatively,
  // together with the node record (slots past numChildren are ignored), saving
  // a dependent round trip; wider speculation would touch cold lines.  Each
  // level's loads are issued before anything waits on the previous level.
  auto loadE0 = [&](int node) {
    return v.lane < SPEC_EDGES && v.lane < v.d.P ? v.inlineEdges(node)[v.lane] : Edge{0u, 0u, 0.0f, 0u};
  };
  Edge e0 = loadE0(ni);
  Node n = v.nodes()[ni];
  // the node an expansion will take (one expansion ends a descent)
  const int freeIdx = s.freeTop > 0 ? (int)v.freeList()[s.freeTop - 1] : -1;
  if(!VL || loadRootPol) {
    // the root's noised policy into LDS: the root selection gathers it per child and
    // scans it for the best unexpanded move
    const float* rn = v.rootNoised();
    float pr[NI];
#pragma unroll
    for(int j = 0; j < NI; j++) {
      const int p = v.lane + 64 * j;
      pr[j] = p < v.d.P ? rn[p] : 0.0f;
    }
#pragma unroll
    for(int j = 0; j < NI; j++) {
      const int p = v.lane + 64 * j;
      if(p < v.d.P)
        rootPol[p] = pr[j];
    }
    waveSync();
  }
  while(true) {
    {
      const unsigned long long tw = SPROF_NOW();
      (void)tw;
      SPROF_WAIT();
      SPROF_ADD(32, SPROF_NOW() - tw);
      SPROF_ADD(35, 1);
    }
    if(n.flags & 2) {
      s.leafKind = LEAF_TERMINAL;
      s.leafNode = ni;
      s.leaf = b;
      break;
    }
    const bool isRoot = ni == s.rootIdx;
    const float* pol = isRoot ? rootPol : v.pol(ni);
    int newPos = -1;
    scanned += n.numChildren;
    const unsigned long long tSel = SPROF_NOW();
    Edge ce{0u, 0u, 0.0f, 0u};
    uint32_t cVisits = 0, cFlags = 0;
    // a node with at most 64 children (every non-root level in practice, the root until
    // its 65th child) takes the one-item form: an empty second item adds nothing to the
    // sums and never wins the (value, index) argmax, so the results are the same
    int slot = n.numChildren <= 64
                   ? selectBest<1, EXPL, VL>(v, s, ni, n, pol, isRoot, newPos, hasBits, e0, ce, cVisits, cFlags)
                   : selectBest<NI, EXPL, VL>(v, s, ni, n, pol, isRoot, newPos, hasBits, e0, ce, cVisits, cFlags);
    SPROF_ADD(5, SPROF_NOW() - tSel);
    (void)tSel;
    if(slot < 0) {
      s.leafKind = LEAF_NOCHILD;
      s.leafNode = ni;
      break;
    }
    if(slot == n.numChildren) {
      const unsigned long long tExp = SPROF_NOW();
      (void)tExp;
      // the node's policy (non-root: the scan for its following expansion candidate) or
      // the root move's raw prior, requested first: the loads fly while the move is
      // played and the SVB / transposition probes run, and are consumed afterwards
      float pvn[NI];
      float rootPrior = 0.0f;
      {
        const float* pp = v.pol(ni);
#pragma unroll
        for(int j = 0; j < NI; j++) {
          const int p = v.lane + 64 * j;
          pvn[j] = !isRoot && p < v.d.P ? pp[p] : -1.0f;
        }
        if(isRoot)
          rootPrior = pp[newPos];
      }
      // child slot `slot` past the inline ones lives in the node's edge-pool block,
      // allocated (16 -> 64 slots) or grown (-> P) here; pool exhaustion ends the
      // descent like node-pool exhaustion (a counted device error)
      uint32_t ebase = n.edgeBase;
      int reserved = 0;  // pool entries taken for this expansion (returned if it fails)
      if(slot == INLINE_EDGES || (slot == 64 && v.d.P > 64)) {
        const int need = edgeBlockCap(slot + 1, v.d.P);
        if(s.edgeTop + need > v.d.edgePoolCap) {
          s.err = ERR_EDGE_POOL;
          s.leafKind = LEAF_NOCHILD;
          s.leafNode = ni;
          break;
        }
        const uint32_t nb = (uint32_t)s.edgeTop;
        s.edgeTop += need;
        s.edgePeak = max(s.edgePeak, s.edgeTop);
        reserved = need;
        if(slot > INLINE_EDGES) {
          Edge* pool = v.edgePool();
          for(int i = v.lane; i < slot - INLINE_EDGES; i += 64)
            pool[nb + i] = pool[ebase + i];
        }
        ebase = nb;
      }
      const float prior = isRoot ? rootPrior : n.nextPrior;
      const int cell = newPos % T.A, dir = newPos / T.A;
      // SVB key of the expansion (needs the board before the move); computed
      // up front so no second board copy stays live across playMoveWave.
      const bool svbKeyed = sp.svbFactor != 0.0f && hCell(b, 0) >= 0;
      uint64_t svbKey = 0, svbFirst = 0;
      if(svbKeyed) {
        svbKey = svbKeyOf<W1>(v, b, hDir(b, 0) * T.A + hCell(b, 0), newPos, b.pla);
        svbFirst = svbProbe(v, s.svbSel, svbKey);
      }
      playMoveWave<W1>(T, b, cell, dir);
      uint64_t k0, k1;
      stateHash(T, b, k0, k1);
      int ttSlot = -1;
      int child = sp.useGraph ? ttFind(v, k0, k1, ttSlot) : -1;
      const bool fresh = child < 0;
      if constexpr(VL) {
        // a transposition onto a node in flight: the playout fails before the edge exists
        if(!fresh && (v.nodes()[child].flags & 3) == 0) {
          s.edgeTop -= reserved;
          if(v.lane == 0) {  // where it collided, past the path's end (coffee_analysis_round_paths)
            v.pathNode()[s.pathLen] = ni;
            v.pathSlot()[s.pathLen] = slot;
          }
          s.leafKind = LEAF_COLLISION;
          s.leafNode = ni;
          break;
        }
      }
      float nxtPrior = -1.0f;
      int nxtPos = 0xFFFF;
      if(!isRoot)
        nextExpansion<NI>(v, pvn, n.nextPrior, n.nextPos, nxtPrior, nxtPos);
      if(fresh) {
        child = allocNode(v, s, b.pla, k0, k1, b.finished != 0, freeIdx);
        if(child < 0) {
          s.edgeTop -= reserved;  // the block was never linked to the node
          s.leafKind = LEAF_NOCHILD;
          s.leafNode = ni;
          break;
        }
        if(svbKeyed) {
          int e = svbFindOrInsert(v, s.svbSel, svbKey, svbFirst);
          waveSync();
          if(v.lane == 0)
            v.nodes()[child].svbEntry = e;
        }
        if(sp.useGraph)
          ttInsertAt(v, ttSlot, k0, k1, child);
      }
      waveSync();
      if(v.lane == 0) {
        v.edges(ni, ebase)[slot] = Edge{(uint32_t)child, 0u, prior, (uint32_t)newPos};
        v.nodes()[ni].numChildren = (uint16_t)(slot + 1);
        v.nodes()[ni].edgeBase = ebase;
        if(!isRoot) {
          v.nodes()[ni].nextPos = (uint16_t)nxtPos;
          v.nodes()[ni].nextPrior = nxtPrior;
        }
        v.pathNode()[s.pathLen] = ni;
        v.pathSlot()[s.pathLen] = slot;
      }
      pushLevel<VL>(s);
      waveSync();
      if constexpr(VL)
        addVirtualLoss(v, child);
      SPROF_ADD(6, SPROF_NOW() - tExp);
      // a fresh node has no visits and the terminal flag of b; a transposition's
      // record is read
      const uint32_t cv = fresh ? 0u : v.nodes()[child].visits;
      const uint32_t cf = fresh ? (b.finished ? 2u : 0u) : (uint32_t)v.nodes()[child].flags;
      if(cv > 0) {
        s.leafKind = LEAF_CATCHUP;
        s.leafNode = child;
        break;
      }
      s.leafNode = child;
      s.leaf = b;
      s.leafKind = (cf & 2) ? LEAF_TERMINAL : LEAF_NN;
      break;
    }
    const int child = (int)ce.child;
    if constexpr(VL) {
      if((cFlags & 3) == 0) {  // in flight (no node without visits is expanded)
        if(v.lane == 0) {
          v.pathNode()[s.pathLen] = ni;
          v.pathSlot()[s.pathLen] = slot;
        }
        s.leafKind = LEAF_COLLISION;
        s.leafNode = ni;
        break;
      }
    }
    if(v.lane == 0) {
      v.pathNode()[s.pathLen] = ni;
      v.pathSlot()[s.pathLen] = slot;
    }
    pushLevel<VL>(s);
    if constexpr(VL)
      addVirtualLoss(v, child);
    if(ce.visits < cVisits) {
      s.leafKind = LEAF_CATCHUP;
      s.leafNode = child;
      break;
    }
    // existing child: its terminal flag already says whether the move ends the game
    const int mv = (int)ce.move, mover = b.pla;
    applyMove<W1>(T, b, mv % T.A, mv / T.A);
    if(cFlags & 2) {
      b.finished = 1;
      b.winner = maxRun<W1>(T, b, mv % T.A) >= T.W ? mover : 0;
    }
    ni = child;
    e0 = loadE0(ni);
    n = v.nodes()[ni];
  }
  s.treeLevels += (uint64_t)s.pathLen;
  s.treeChildren += scanned;
}

// ---------------------------------------------------------------------------
// kSelect: root evaluation or one descent; NN leaves are encoded into the batch.

// NN evaluation cache lookup of an NN leaf (SPEC a7): a state evaluated in an earlier
// round by any game is taken from the cache instead of the network.  The payload is
// loaded with the key and a hit copies it into the leaf's policy.  fused (kBackupSelect):
// the slot's tag is loaded too -- a bid of this round (tag != 0) means this round's
// backups, running beside this selection, write the slot, so the lookup is left to
// kResolve (LEAF_PENDING); any other slot is not written during the kernel.
//
// Match play (the MATCH instantiations; DESIGN.md "Match play"): each of the two nets has
// its own cache, as the reference has one per NNEvaluator.  netOf is the one place the net
// of a game's evaluations -- and with it the cache -- is derived: the compaction, the
// lookup and the cache write all go through it.  The root and the game number it reads
// change only in kCommit (and in a policy-initialisation backup, after its evaluation is
// consumed), so a round's select, compaction and backup agree, also for a deferred row.
// With a shared net (matchSharedNet) both sides are net 0: one list, one cache, one launch.
KC_D int netOf(const SearchDev& d, int g, const GameDev& s) {
  return d.matchSharedNet ? 0 : sideOf(d, g, s);
}
struct NNCache {
  uint64_t* key;
  float* pol;
  float* val;
  float* err;
  uint32_t* tag;
};
// The cache of net `net`; without MATCH the single one, whatever `net`.
template <bool MATCH>
KC_D NNCache cacheOf(const SearchDev& d, int net) {
  if constexpr(MATCH) {
    if(net != 0)
      return NNCache{d.cKey1, d.cPol1, d.cVal1, d.cErr1, d.cTag1};
  }
  return NNCache{d.cKey, d.cPol, d.cVal, d.cErr, d.cTag};
}

template <int NI, bool MATCH = false>
KC_D void cacheLookup(const GV& v, GameDev& s, bool fused) {
  const SearchDev& d = v.d;
  const NNCache c = cacheOf<MATCH>(d, MATCH ? netOf(d, v.g, s) : 0);
  const uint64_t k0 = v.nodeKey(s.leafNode)[0], k1 = v.nodeKey(s.leafNode)[1];
  const uint32_t slot = cacheSlot(k0, k1, d.cacheMask);
  const int P = d.P;
  const float* cp = c.pol + (size_t)slot * P;
  float pv[NI];
#pragma unroll
  for(int j = 0; j < NI; j++) {
    const int pos = v.lane + 64 * j;
    pv[j] = pos < P ? cp[pos] : 0.0f;
  }
  const float cw = c.val[2 * (size_t)slot], cl = c.val[2 * (size_t)slot + 1], ce = c.err[slot];
  const uint32_t tag = fused ? c.tag[slot] : 0u;
  s.cSlot = (int32_t)slot;
  if(tag != 0u) {
    s.leafKind = LEAF_PENDING;
    if(v.lane == 0)
      d.pendList[atomicAdd(d.pendCount, 1)] = v.g;  // rare: a same-round transposition
    return;
  }
  if(c.key[2 * (size_t)slot] == k0 && c.key[2 * (size_t)slot + 1] == k1) {
    s.leafKind = LEAF_CACHED;
    s.cHitWin = cw;
    s.cHitLoss = cl;
    s.cHitErr = ce;
    float* pol = v.pol(s.leafNode);
#pragma unroll
    for(int j = 0; j < NI; j++) {
      const int pos = v.lane + 64 * j;
      if(pos < P)
        pol[pos] = pv[j];
    }
  }
}

// The end of a descent or of another phase's evaluation request: an NN leaf draws its symmetry
// and the playout's batch row (GV::row) is encoded when the leaf needs the network.
template <bool W1>
KC_D void finishLeaf(const GV& v, GameDev& s, DRng& rng) {
  const SearchDev& d = v.d;
  if(s.leafKind == LEAF_NN)
    s.leafSym = (int)rng.below(8);
  s.rngCtr = rng.ctr;
  const bool needNN =
      s.leafKind == LEAF_NN || s.leafKind == LEAF_ROOTEVAL || s.leafKind == LEAF_INIT || s.leafKind == LEAF_FORK ||
      s.leafKind == LEAF_SIDE;
  if(v.lane == 0) {
    d.nnNeed[v.row] = needNN ? 1 : 0;
    if(needNN)
      d.nnBid[v.row] = s.leafKind == LEAF_NN && d.cacheOn ? (uint32_t)s.cSlot : ~0u;
  }
  if(needNN) {
    // the game's own batch row: no shared counter (a same-address atomic from
    // every block serialises at L2); kCompact lists the rows the network evaluates
    const int slot = v.row;
    s.nnSlot = slot;
    s.nnEvals++;
    encodePackedWave<W1>(v.T, s.leaf, s.leafSym, d.nnIn + (size_t)slot * d.inWords);
  }
}

// The end of a selection: finishLeaf, and the game state is stored.
template <bool W1>
KC_D void finishSelect(const GV& v, GameDev& s, DRng& rng) {
  finishLeaf<W1>(v, s, rng);
  waveSync();
  storeGame(v, s);
}

// One game's selection.  s: the game's LDS copy, already holding its state when `loaded`
// (the fused kernel's backup just ran; every path below then stores it).  rootPol: LDS [MAX_P].
template <int NI, bool MATCH = false, bool EXPL = false>
KC_D void selectBody(const SearchDev& d, const DTables& T, int g, GameDev& s, bool loaded, bool fused,
                     uint32_t* hasBits, float* rootPol, int row = -1) {
  GV v(d, T, g);
  if(row >= 0)  // a wide engine's rows: the slot's first
    v.row = row;
  SPROF_INIT();
  const unsigned long long t0 = SPROF_NOW();
  if(d.nnDefer[g]) {
    // the leaf from an earlier round still waits for the network (kCompact); the
    // game state stays as it is
    if(v.lane == 0)
      d.nnNeed[v.row] = 1;
    return;
  }
  if(loaded)
    bindGame<MATCH>(v, s);
  else
    loadGame<MATCH>(v, s);
  if(s.phase == PH_COMMIT || s.startDelay > 0) {
    s.leafKind = LEAF_NONE;
    if(loaded) {
      // the fused kernel's backup left the state to be stored here
      if(s.startDelay > 0)
        s.startDelay = s.startDelay - 1;
      storeGame(v, s);
      if(v.lane == 0)
        d.nnNeed[v.row] = 0;
      return;
    }
    if(v.lane == 0) {
      d.games[g].leafKind = LEAF_NONE;
      if(s.startDelay > 0)
        d.games[g].startDelay = s.startDelay - 1;
      d.nnNeed[v.row] = 0;
    }
    return;
  }
  const unsigned long long t1 = SPROF_NOW();
  (void)t0;
  (void)t1;
  DRng rng = DRng{s.rngSeed, s.rngCtr};
  if(s.phase == PH_INIT) {
    // policy-initialisation move: one evaluation of the root, random symmetry
    s.leafKind = LEAF_INIT;
    s.leafSym = (int)rng.below(8);
    s.leaf = s.root;
  } else if(s.phase == PH_SIDEEVAL) {
    // side-position continuation: the position after the search's response (set by
    // kCommit in s.leaf), random symmetry
    s.leafKind = LEAF_SIDE;
    s.leafSym = (int)rng.below(8);
  } else if(s.phase == PH_FORK) {
    // fork candidate: the position after the next candidate move, random symmetry
    const ForkRec* f = d.fork + g;
    const int mv = f->moves[f->next];
    s.leaf = f->board;
    playMoveWave(v.T, s.leaf, mv % v.T.A, mv / v.T.A);
    s.leafKind = LEAF_FORK;
    s.leafSym = (int)rng.below(8);
  } else if(s.phase == PH_ROOTEVAL) {
    if(s.rootK == 0) {
      // partial Fisher-Yates over 0..7, kept as packed nibbles (no dynamic register indexing)
      uint32_t idx = 0x76543210u;
#pragma unroll
      for(int k = 0; k < 4; k++) {
        int j = k + (int)rng.below((uint32_t)(8 - k));
        uint32_t a = (idx >> (4 * k)) & 15u, b = (idx >> (4 * j)) & 15u;
        idx = (idx & ~(15u << (4 * k)) & ~(15u << (4 * j))) | (b << (4 * k)) | (a << (4 * j));
      }
      s.syms = idx & 0xFFFFu;
    }
    s.leafKind = LEAF_ROOTEVAL;
    s.leafSym = (int)((s.syms >> (4 * s.rootK)) & 15u);
    s.leaf = s.root;
  } else {
    descend<NI, EXPL>(v, s, hasBits, rootPol);
    if(s.leafKind == LEAF_NN && d.cacheOn)
      cacheLookup<NI, MATCH>(v, s, fused);
  }
  const unsigned long long t2 = SPROF_NOW();
  (void)t2;
  finishSelect<W1_OF<NI>>(v, s, rng);
  SPROF_ADD(0, 1);
  SPROF_MAX(24, SPROF_NOW() - t0);
  SPROF_MAX(25, s.pathLen);
  SPROF_ADD(1, SPROF_NOW() - t0);
  SPROF_ADD(2, t1 - t0);
  SPROF_ADD(3, t2 - t1);
  SPROF_ADD(4, s.pathLen);
  SPROF_ADD(7, SPROF_NOW() - t2);
  SPROF_FLUSH();
}

template <int NI, bool MATCH = false, bool EXPL = false>
__global__ void __launch_bounds__(64, NI <= 2 ? 4 : 2) kSelect(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp,
                                                                int resetCommit) {
  const SearchDev& d = *dp;
  const int g = blockIdx.x;
  // the previous commit's list is consumed (kCommit/kRows ran before this kernel);
  // this round's kBackup appends to an empty one
  if(resetCommit && g == 0 && threadIdx.x == 0)
    *d.commitCount = 0;
  if(g >= d.G)
    return;
  __shared__ uint32_t hasBits[(MAX_P + 31) / 32];
  __shared__ GameDev s;
  __shared__ float rootPol[MAX_P];
  selectBody<NI, MATCH, EXPL>(d, *Tp, g, s, false, false, hasBits, rootPol);
}

// The selections a fused kernel left pending: the cache slot is final now (every backup
// of the round has run), so the lookup and the rest of the selection complete here, in
// the order kSelect runs them (the symmetry draw comes after the lookup).  Each round
// winner's tag is cleared too (before the next kCompact bids).  A small grid: block b
// clears the tags of games b, b + grid, ... and completes pending entries b, b + grid, ...
constexpr int RESOLVE_GRID = 64;
// The two halves of a resolve, shared by kResolve and the resolving kCompact: clearing
// the round winners' tags (entries first, first + stride, ...) and completing the pending
// selections (entries first, first + stride, ...; one wave each, s its LDS game copy).
KC_D void clearRoundTags(const SearchDev& d, int first, int stride) {
  for(int i = first; i < d.G; i += stride) {
    const uint32_t cc = d.cClear[i];
    if(cc != 0u) {
      d.cTag[cc - 1u] = 0u;
      d.cClear[i] = 0u;
    }
  }
}
template <int NI>
KC_D void completePending(const SearchDev& d, const DTables& T, int first, int stride, GameDev& s) {
  const int np = *d.pendCount;
  for(int k = first; k < np; k += stride) {
    const int g = __builtin_amdgcn_readfirstlane(d.pendList[k]);
    GV v(d, T, g);
    loadGame(v, s);
    s.leafKind = LEAF_NN;
    cacheLookup<NI>(v, s, false);
    DRng rng = DRng{s.rngSeed, s.rngCtr};
    finishSelect<W1_OF<NI>>(v, s, rng);
  }
}
template <int NI>
__global__ void __launch_bounds__(64) kResolve(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  const SearchDev& d = *dp;
  clearRoundTags(d, blockIdx.x * 64 + laneId(), RESOLVE_GRID * 64);
  __shared__ GameDev s;
  completePending<NI>(d, *Tp, blockIdx.x, RESOLVE_GRID, s);
}

// oracle postprocess (nneval.cpp:702-815 + copyOutputsWithSymmetry nninputs.cpp:349-357)
template <int NI>
// The network row is staged in LDS (one coalesced read) and gathered from there in
// the symmetric frame; pv returns each lane's policy values for buildOrder.
// `stage` (>= P+4 floats) may alias polDst.  stLogit: the row's short-term win/loss error
// logit out[P+3] (uncertainty weighting; the callers that need no weight drop it).
KC_D void postprocess(const GV& v, const DBoard& b, int sym, const float* out, float* polDst, float& whiteWin,
                      float& whiteLoss, float& stLogit, float* stage, float (&pv)[NI]) {
  const DTables& T = v.T;
  const int P = T.P, A = T.A;
  if(T.X != T.Y)
    sym &= 3;
  float raw[NI + 1];
#pragma unroll
  for(int j = 0; j <= NI; j++) {
    const int i = v.lane + 64 * j;
    raw[j] = i < P + 4 ? out[i] : 0.0f;
  }
  int src[NI];
  bool legal[NI];
#pragma unroll
  for(int j = 0; j < NI; j++) {
    const int pos = v.lane + 64 * j;
    legal[j] = false;
    src[j] = 0;
    if(pos < P) {
      const int dd = pos / A, cell = pos % A;
      legal[j] = isLegal<W1_OF<NI>>(T, b, cell, dd);
      src[j] = T.symDir[sym][dd] * A + T.symCell[sym][cell];
    }
  }
  waveSync();
#pragma unroll
  for(int j = 0; j <= NI; j++) {
    const int i = v.lane + 64 * j;
    if(i < P + 4)
      stage[i] = raw[j];
  }
  waveSync();
  float logit[NI];
  float mx = -1e25f;
  int legalCount = 0;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    const int pos = v.lane + 64 * j;
    logit[j] = -1e30f;
    if(pos < P) {
      logit[j] = legal[j] ? stage[src[j]] : -1e30f;
      mx = logit[j] > mx ? logit[j] : mx;
    }
    legalCount += __popcll(ballot(legal[j]));
  }
  const float wlg = stage[P], llg = stage[P + 1];
  stLogit = stage[P + 3];
  waveSync();
  mx = waveMax(mx);
  float e[NI];
#pragma unroll
  for(int j = 0; j < NI; j++)
    e[j] = dexp(logit[j] - mx);
  const float sum = tsum<NI>(e, P, v.lane);
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int pos = v.lane + 64 * j;
    pv[j] = legal[j] ? (sum <= 0.0f ? 1.0f / (float)legalCount : e[j] / sum) : -1.0f;
    if(pos < P)
      polDst[pos] = pv[j];
  }
  float m = wlg > llg ? wlg : llg;
  float wp = dexp(wlg - m), lp = dexp(llg - m);
  float ps = wp + lp;
  wp = wp / ps;
  lp = lp / ps;
  if(b.pla == 2) {
    whiteWin = wp;
    whiteLoss = lp;
  } else {
    whiteWin = lp;
    whiteLoss = wp;
  }
}

KC_D float interpolateEarly(const DTables& T, int turn, float halflife, float earlyValue, float value) {
  float rawHalflives = (float)turn / halflife;
  float halflives = rawHalflives * (19.0f / sqrtf((float)(T.X * T.Y)));
  return value + (earlyValue - value) * dpow(0.5f, halflives);
}

// Sequential in-order sum of lds[0..n) (the oracle's plain loops), result to all lanes.
KC_D float seqSum(float* lds, int n, int lane) {
  waveSync();
  float acc = 0.0f;
  if(lane == 0)
    for(int i = 0; i < n; i++)
      acc = acc + lds[i];
  return bcastLaneF(acc, 0);
}

// oracle noiseAndTemp (maybeAddPolicyNoiseAndTemp searchhelpers.cpp:122-222)
KC_D void noiseAndTemp(const GV& v, GameDev& s, DRng& rng, const float* raw, float* out, float* scratch) {
  const SP& sp = *v.sp;
  const int P = v.d.P;
  for(int pos = v.lane; pos < P; pos += 64)
    out[pos] = raw[pos];
  waveSync();
  if(sp.rootTemp != 1.0f || sp.rootTempEarly != 1.0f) {
    float t = interpolateEarly(v.T, s.root.turn, sp.moveTempHalflife, sp.rootTempEarly, sp.rootTemp);
    float mx = 0.0f;
    for(int pos = v.lane; pos < P; pos += 64)
      mx = out[pos] > mx ? out[pos] : mx;
    mx = waveMax(mx);
    float logMax = dlog(mx);
    float invTemp = 1.0f / t;
    for(int pos = v.lane; pos < P; pos += 64) {
      float o = out[pos];
      float p = 0.0f;
      if(o > 0.0f) {
        p = dexp((dlog(o) - logMax) * invTemp);
        out[pos] = p;
      }
      scratch[pos] = p;  // zero terms do not change the in-order sum
    }
    float sum = seqSum(scratch, P, v.lane);
    waveSync();
    for(int pos = v.lane; pos < P; pos += 64)
      if(out[pos] >= 0.0f)
        out[pos] = out[pos] / sum;
    waveSync();
  }
  if(sp.rootNoise) {
    // computeDirichletAlphaDistribution searchhelpers.cpp:51-91
    int legalCount = 0;
    for(int base = 0; base < P; base += 64) {
      int pos = base + v.lane;
      legalCount += __popcll(ballot(pos < P && out[pos] >= 0.0f));
    }
    float* alpha = scratch;          // [P]
    float* r = scratch + MAX_P;      // [P]
    for(int pos = v.lane; pos < P; pos += 64)
      alpha[pos] = out[pos] >= 0.0f ? dlog(fminf(0.01f, out[pos]) + 1e-20f) : 0.0f;
    float logSum = seqSum(alpha, P, v.lane);
    float logMean = logSum / (float)legalCount;
    waveSync();
    for(int pos = v.lane; pos < P; pos += 64)
      alpha[pos] = out[pos] >= 0.0f ? fmaxf(0.0f, alpha[pos] - logMean) : 0.0f;
    float propSum = seqSum(alpha, P, v.lane);
    float uniform = 1.0f / (float)legalCount;
    waveSync();
    for(int pos = v.lane; pos < P; pos += 64)
      if(out[pos] >= 0.0f)
        alpha[pos] = propSum <= 0.0f ? uniform : 0.5f * (alpha[pos] / propSum + uniform);
    // addDirichletNoise searchhelpers.cpp:93-120; SPEC a24 per-move sub-streams
    const uint64_t base = rng.next();
    for(int pos = v.lane; pos < P; pos += 64) {
      float rv = 0.0f;
      if(out[pos] >= 0.0f) {
        DRng sub{mix64(base ^ ((uint64_t)(pos + 1) * 0x9e3779b97f4a7c15ULL)), 0};
        rv = sub.gamma(alpha[pos] * sp.dirConc);
      }
      r[pos] = rv;
    }
    float rSum = seqSum(r, P, v.lane);
    waveSync();
    float w = sp.dirWeight;
    for(int pos = v.lane; pos < P; pos += 64) {
      float rr = r[pos] / rSum;
      if(out[pos] >= 0.0f)
        out[pos] = rr * w + out[pos] * (1.0f - w);
    }
    waveSync();
  }
}

// A freshly evaluated node's first expansion candidate.
template <int NI>
KC_D void firstExpansion(const GV& v, int ni, const float (&pv)[NI]) {
  float pr;
  int pos;
  nextExpansion<NI>(v, pv, __builtin_inff(), -1, pr, pos);
  if(v.lane == 0) {
    v.nodes()[ni].nextPos = (uint16_t)pos;
    v.nodes()[ni].nextPrior = pr;
  }
  waveSync();
}

// kBackup: NN post-processing + leaf value + path backup.
KC_D bool setMoveLimits(const GV& v, GameDev& s, DRng& rng, float lastWL);
template <bool MATCH = false>
KC_D void finishGameRecord(const GV& v, const GameDev& s, DRng& rng, float* scratch);
KC_D void startGame(const GV& v, GameDev& s, bool deferTurns = false);
template <int NI>
KC_D void forkEval(const GV& v, GameDev& s, const float* o, float* scratch);
template <int NI>
KC_D void sideEval(const GV& v, GameDev& s, const float* o, float* scratch);

// oracle initMove (getGameInitializationMove playutils.cpp:97-145 + the move of
// initializeGameUsingPolicy :163-175): a move sampled from the root's post-processed
// policy raised to 1/temperature (2e-4 of the time uniformly among the candidates),
// played without search and recorded as a turn without rows.  Returns true when the
// move ended the game (kCommit then finishes it).
template <int NI>
KC_D bool initMove(const GV& v, GameDev& s, const float* o, float* scratch /* LDS [2*MAX_P] */) {
  const SP& b = v.d.sp;
  const int P = v.d.P, A = v.T.A;
  float* pol = scratch;
  float w, l, st;
  float pv[NI];
  postprocess<NI>(v, s.root, s.leafSym, o, pol, w, l, st, scratch, pv);
  waveSync();
  // candidates in ascending policy position: legal with probability > 0
  int* cpos = reinterpret_cast<int*>(scratch + MAX_P);
  float* cval = scratch;  // overwrites pol in place: candidate i <= its position
  int n = 0;
  const float invT = 1.0f / b.initTemp;
  for(int base = 0; base < P; base += 64) {
    const int p = base + v.lane;
    const float q = p < P ? pol[p] : -1.0f;
    const bool ok = q > 0.0f;
    const uint64_t m = ballot(ok);
    waveSync();
    if(ok) {
      const int i = n + __popcll(m & ((1ULL << v.lane) - 1ULL));
      cpos[i] = p;
      cval[i] = b.initTemp == 1.0f ? q : dpow(q, invT);
    }
    n += __popcll(m);
    waveSync();
  }
  DRng rng{s.rngSeed, s.rngCtr};
  int idx = 0;
  if(rng.uni() < 0.0002f) {
    idx = (int)rng.below((uint32_t)n);
  } else {
    const float sum = seqSum(cval, n, v.lane);
    const float dd = rng.uni() * sum;
    idx = n - 1;
    if(v.lane == 0) {
      float acc = 0.0f;
      for(int i = 0; i < n; i++) {
        acc = acc + cval[i];
        if(acc > dd) {
          idx = i;
          break;
        }
      }
    }
    idx = bcastI(idx, 0);
  }
  s.rngCtr = rng.ctr;
  const int chosen = cpos[idx];
  waveSync();
  if(v.lane == 0) {
    TurnRec rec;
    memset(&rec, 0, sizeof(rec));
    rec.gen = (uint8_t)*v.d.modelGen;
    rec.cell = (int8_t)(chosen % A);
    rec.dir = (int8_t)(chosen / A);
    v.turns()[s.numTurns] = rec;
  }
  s.numTurns++;
  s.startTurn++;
  s.initLeft--;
  playMoveWave(v.T, s.root, chosen % A, chosen / A);
  waveSync();
  if(s.root.finished)
    return true;
  if(s.initLeft == 0) {
    DRng r2{s.rngSeed, s.rngCtr};
    setMoveLimits(v, s, r2, 0.0f);
    s.rngCtr = r2.ctr;
    s.phase = PH_ROOTEVAL;
    s.rootK = 0;
  }
  return false;
}

// The evaluations that are not playouts -- a policy-initialisation move, a fork candidate,
// a side position, one symmetry of a root evaluation (a few per move against hundreds of
// playouts) -- run out of line: the round kernels' straight line and register allocation
// do not carry them.  Arguments by value; the game's state goes through its LDS copy *gs
// (the fences order this function's generic-pointer accesses to it against the caller's).
// Returns whether the game is due for a commit.
template <class T>
KC_D T* uniformPtr(T* p) {  // a function's arguments arrive per lane: back to a scalar
  const uint64_t x = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
  return (T*)(((uint64_t)hi << 32) | lo);
}
// A uniform pointer to a structure no kernel writes (SearchDev, DTables), as a constant-
// address-space pointer: its uniform reads stay scalar loads inside a called function, as
// they are through the kernels' readonly arguments (asGlobal in search.h needs them so).
template <class T>
KC_D const T* uniformConst(const T* p) {
  const __attribute__((address_space(4))) T* q = (const __attribute__((address_space(4))) T*)uniformPtr(p);
  asm volatile("" : "+s"(q));
  return (const T*)q;
}
// (EXPL: nothing here reads it; it gives each round kernel the out-of-line copy of its own
// instantiation family, as MATCH does, so a copy's callers -- and with them what the compiler
// propagates into it -- stay the ones it had before the exploration kernels existed; WIDE likewise
// for the wide kernels)
template <int NI, bool MATCH = false, bool EXPL = false, bool WIDE = false>
__device__ __noinline__ bool rareLeaf(const SearchDev* dp, const DTables* Tp, int g, GameDev* gs, float* scratch) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const SearchDev& d = *uniformConst(dp);
  GameDev& s = *uniformPtr(gs);
  scratch = uniformPtr(scratch);
  g = __builtin_amdgcn_readfirstlane(g);
  GV v(d, *uniformConst(Tp), g);
  bindGame<MATCH>(v, s);
  const SP& sp = *v.sp;
  const int P = d.P;
  const float* o = d.nnOut + (size_t)s.nnSlot * (P + 4);
  bool needCommit = false;
  if(s.leafKind == LEAF_INIT) {
    needCommit = initMove<NI>(v, s, o, scratch);
    matchMoveLimits<MATCH>(v, s);  // the first searched move's limit, by its mover
  } else if(s.leafKind == LEAF_FORK) {
    forkEval<NI>(v, s, o, scratch);
  } else if(s.leafKind == LEAF_SIDE) {
    sideEval<NI>(v, s, o, scratch);
  } else {
    float* pol = scratch;
    float w, l, st;
    float pv[NI];
    postprocess<NI>(v, s.root, s.leafSym, o, pol, w, l, st, scratch, pv);
    waveSync();
    // the short-term error is averaged over the sampled symmetries like win / loss
    // (nninputs.cpp:108-119); the root's weight comes from the average
    const float err = v.unc->on ? stErrorOf(st) : 0.0f;
    float* acc = v.accPolicy();
    if(s.rootK == 0) {
      for(int p = v.lane; p < P; p += 64) {
        v.rawPolicy()[p] = pol[p];
        acc[p] = 0.0f + pol[p];
      }
      s.rawWin = w;
      s.rawLoss = l;
      s.accWin = 0.0f + w;
      s.accLoss = 0.0f + l;
      s.accErr = 0.0f + err;
    } else {
      for(int p = v.lane; p < P; p += 64)
        acc[p] = acc[p] + pol[p];
      s.accWin = s.accWin + w;
      s.accLoss = s.accLoss + l;
      s.accErr = s.accErr + err;
    }
    s.rootK++;
    if(s.rootK == sp.rootSyms) {
      const float fl = (float)sp.rootSyms;
      const bool fresh = s.rootIdx < 0;
      if(fresh) {
        uint64_t k0, k1;
        stateHash(v.T, s.root, k0, k1);
        s.rootIdx = allocNode(v, s, s.root.pla, k0, k1, false);
      }
      waveSync();
      float* rp = v.pol(s.rootIdx);
      for(int p = v.lane; p < P; p += 64)
        rp[p] = acc[p] / fl;
      if(v.lane == 0) {
        Node* r = &v.nodes()[s.rootIdx];
        r->nnWin = s.accWin / fl;
        r->nnLoss = s.accLoss / fl;
        r->nnWeight = uncWeightOf(*v.unc, s.accErr / fl);
        r->flags |= 1;
      }
      waveSync();
      if(fresh) {
        const Node& r = v.nodes()[s.rootIdx];
        addLeafValue(v, s, s.rootIdx, r.nnWin - r.nnLoss, r.nnWeight, false, true);
      }
      DRng rng{s.rngSeed, s.rngCtr};
      noiseAndTemp(v, s, rng, rp, v.rootNoised(), scratch);
      s.rngCtr = rng.ctr;
      // analysis: the query's masked root moves (analysisRefill) leave the noised policy, after
      // noise and temperature were drawn over every legal move -- the root selection skips
      // entries below 0 among its children and in its scan for the next one
      if(d.rootMask.p != nullptr) {
        const uint32_t* mk = d.rootMask + (size_t)g * ((P + 31) >> 5);
        float* rn = v.rootNoised();
        waveSync();
        for(int p = v.lane; p < P; p += 64)
          if((mk[p >> 5] >> (p & 31)) & 1u)
            rn[p] = -1.0f;
      }
      s.phase = PH_SEARCH;
      needCommit = v.nodes()[s.rootIdx].visits >= (uint32_t)s.visitLimit;
    }
  }
  waveSync();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  return needCommit;
}

// One playout's backup: the leaf takes its evaluation (post-processed from the playout's network
// row, or the cache hit's) or its terminal / repeated value, and the path is backed up.
// The NN-cache slot the evaluation bid for is written by the round's highest bidding row.
// P, o: d.P and the playout's network output row (the caller has both at hand).
template <int NI, bool MATCH = false, bool EXPL = false>
KC_D void playoutBackup(const GV& v, GameDev& s, const int P, const float* o, bool fused, float* scratch) {
  const SearchDev& d = v.d;
  const int g = v.g;
  unsigned long long tPost = 0, tLeaf = 0, tPath = 0;
  (void)tPost;
  (void)tLeaf;
  (void)tPath;
  NStats leafSt{0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool haveLeaf = false;
  if(s.leafKind == LEAF_NN || s.leafKind == LEAF_CACHED) {
    float w, l, err = 0.0f;  // err: the evaluation's short-term error (uncertainty weighting)
    float* pol = v.pol(s.leafNode);
    const unsigned long long ta = SPROF_NOW();
    (void)ta;
    float pv[NI];
#ifdef KC_SEARCH_PROFILE
    if(v.lane == 0)
      probeLeafKey(v.nodeKey(s.leafNode)[0], v.nodeKey(s.leafNode)[1]);
#endif
    if(s.leafKind == LEAF_CACHED) {
      // copied from the cache into the leaf's policy by kSelect
#pragma unroll
      for(int j = 0; j < NI; j++) {
        const int pos = v.lane + 64 * j;
        pv[j] = pos < P ? pol[pos] : -1.0f;
      }
      w = s.cHitWin;
      l = s.cHitLoss;
      err = s.cHitErr;
    } else {
      float st;
      postprocess<NI>(v, s.leaf, s.leafSym, o, pol, w, l, st, scratch, pv);
      // MATCH with a shared net: the cache entry written below serves both sides, so it carries the
      // error whenever either side weights by it (the side with the setting off ignores it:
      // uncWeightOf gives 1)
      bool wantErr = v.unc->on != 0;
      if constexpr(MATCH)
        wantErr = wantErr || (d.matchSharedNet && (d.unc.on | d.unc1.on) != 0);
      if(wantErr)
        err = stErrorOf(st);
      if(d.cacheOn) {
        // kCompact bid this evaluation for the state's cache slot (atomicMax of
        // game + 1 over the round's batch); the highest bidder stores its payload
        // and clears the tag, deterministic whatever the block order.  Nothing
        // reads the table in this kernel (hits were copied by kSelect).
        const NNCache c = cacheOf<MATCH>(d, MATCH ? netOf(d, g, s) : 0);
        const uint32_t slot = (uint32_t)s.cSlot;
        if(c.tag[slot] == (uint32_t)v.row + 1u) {
          float* cp = c.pol + (size_t)slot * P;
#pragma unroll
          for(int j = 0; j < NI; j++)
            if(v.lane + 64 * j < P)
              cp[v.lane + 64 * j] = pv[j];
          if(v.lane == 0) {
            c.val[2 * (size_t)slot] = w;
            c.val[2 * (size_t)slot + 1] = l;
            c.err[slot] = err;
            c.key[2 * (size_t)slot] = v.nodeKey(s.leafNode)[0];
            c.key[2 * (size_t)slot + 1] = v.nodeKey(s.leafNode)[1];
            if(fused)
              d.cClear[g] = slot + 1u;
            else
              c.tag[slot] = 0;
          }
        }
      }
    }
    firstExpansion<NI>(v, s.leafNode, pv);
    const float weight = uncWeightOf(*v.unc, err);
    if(v.lane == 0) {
      Node* n = &v.nodes()[s.leafNode];
      n->nnWin = w;
      n->nnLoss = l;
      n->nnWeight = weight;
      n->flags |= 1;
    }
    waveSync();
    const unsigned long long tb = SPROF_NOW();
    (void)tb;
    leafSt = addLeafValue(v, s, s.leafNode, w - l, weight, false, true);
    haveLeaf = true;
    tPost = tb - ta;
    tLeaf = SPROF_NOW() - tb;
  } else if(s.leafKind == LEAF_TERMINAL) {
    float val = s.leaf.winner == 2 ? 1.0f : (s.leaf.winner == 1 ? -1.0f : 0.0f);
    leafSt = addLeafValue(v, s, s.leafNode, val, uncTerminalWeight(*v.unc), true, false);
    haveLeaf = true;
  } else if(s.leafKind == LEAF_NOCHILD) {
    const Node& n = v.nodes()[s.leafNode];
    leafSt = addLeafValue(v, s, s.leafNode, n.nnWin - n.nnLoss, n.nnWeight, false, false);
    haveLeaf = true;
  }
  const unsigned long long tp0 = SPROF_NOW();
  (void)tp0;
  // an updated leaf is the deepest level's path child (a catch-up leaf is unchanged)
  backupPath<NI, EXPL>(v, s, s.pathLen, leafSt, haveLeaf);
  tPath = SPROF_NOW() - tp0;
  s.playouts++;
  SPROF_ADD(12, tPost);
  SPROF_ADD(13, tPath);
  SPROF_ADD(14, tLeaf);
}

// One game's backup; returns whether s holds the game's state afterwards (fused: not yet
// stored -- selectBody stores it on every path).
// fused (kBackupSelect): a cache-slot winner leaves the slot's tag set -- the selections
// running beside it treat the slot as being written -- and kResolve clears it.
template <int NI, bool MATCH = false, bool EXPL = false, bool WIDE = false>
KC_D bool backupBody(const SearchDev& d, const DTables& T, int g, GameDev& s, bool fused, float* scratch) {
  if(d.nnDefer[g])  // a deferred leaf is backed up in a later round
    return false;
  GV v(d, T, g);
  SPROF_INIT();
  const unsigned long long t0 = SPROF_NOW();
  (void)t0;
  loadGame<MATCH>(v, s);
  if(s.leafKind == LEAF_NONE)
    return true;
  const int P = d.P;
  const float* o = d.nnOut + (size_t)s.nnSlot * (P + 4);
  bool needCommit = false;
  if(s.leafKind == LEAF_INIT || s.leafKind == LEAF_FORK || s.leafKind == LEAF_SIDE || s.leafKind == LEAF_ROOTEVAL) {
    needCommit = rareLeaf<NI, MATCH, EXPL, WIDE>(&d, &T, g, &s, scratch);
  } else {
    playoutBackup<NI, MATCH, EXPL>(v, s, P, o, fused, scratch);
    needCommit = v.nodes()[s.rootIdx].visits >= (uint32_t)s.visitLimit;
  }
  if(needCommit) {
    s.phase = PH_COMMIT;
    if(v.lane == 0)
      d.commitList[atomicAdd(d.commitCount, 1)] = g;
  }
  s.leafKind = LEAF_NONE;
  waveSync();
  if(!fused)  // fused: the selection that follows stores the state once (408 B per game less)
    storeGame(v, s);
  SPROF_ADD(10, 1);
  SPROF_MAX(26, SPROF_NOW() - t0);
  SPROF_ADD(11, SPROF_NOW() - t0);
  SPROF_FLUSH();
  return true;
}

template <int NI, bool MATCH = false, bool EXPL = false>
__global__ void __launch_bounds__(64, NI <= 4 ? 4 : 3) kBackup(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  // (constant views: the call to rareLeaf does not count as a write to *dp or *Tp, so
  // their uniform reads after it stay scalar loads)
  const SearchDev& d = *uniformConst(dp);
  const DTables& T = *uniformConst(Tp);
  const int g = blockIdx.x;
  if(g >= d.G)
    return;
  __shared__ __attribute__((aligned(16))) float scratch[3 * MAX_P];
  __shared__ GameDev s;
  backupBody<NI, MATCH, EXPL>(d, T, g, s, false, scratch);
}

// Round r's backup and round r+1's selection of one game in one kernel (no commit between
// them).  Games only read and write their own trees and tables; the one table they share,
// the NN cache, is handled by the tags (backupBody / cacheLookup / kResolve), so every
// result is the one the two separate kernels give.  One kernel boundary less per round,
// and a game's slow backup and slow descent no longer each set a kernel's length.
// At 5x5 the fused kernel is compiled for 4 waves per SIMD (128 VGPRs, as kSelect /
// kBackup; beside a network workgroup's two waves a SIMD holds one such wave.
// 6 (80 VGPRs: two fit) spills 332 B per lane and ran 18.0 k against 24.4 k rows/s, 5
// 21.6 k: profiles/r05/fused_occupancy_ab.txt)
template <int NI, bool EXPL = false>
__global__ void __launch_bounds__(64, NI <= 2 ? 4 : 2) kBackupSelect(const SearchDev* __restrict__ dp,
                                                                     const DTables* __restrict__ Tp) {
  const SearchDev& d = *uniformConst(dp);  // constant views: see kBackup
  const DTables& T = *uniformConst(Tp);
  const int g = blockIdx.x;
  if(g >= d.G)
    return;
  __shared__ __attribute__((aligned(16))) float scratch[3 * MAX_P];
  __shared__ uint32_t hasBits[(MAX_P + 31) / 32];
  __shared__ GameDev s;
  const bool loaded = backupBody<NI, false, EXPL>(d, T, g, s, true, scratch);
  // (the selection's root policy reuses the backup's scratch)
  selectBody<NI, false, EXPL>(d, T, g, s, loaded, true, hasBits, scratch);
}

// ---------------------------------------------------------------------------
// Parallel playouts per search (coffee_analysis_set_search_threads).  With
// wideK = K a searching slot makes up to K descents a round, one after the other on its one
// wave, steered apart by virtual losses (vloss.h); their leaves go through the network in the
// round's one batch, descent j of slot g on row g K + j, and the backups then run in the same
// order.  Between the two kernels descent j's leaf lives in wideRec[g][j] and its path in
// widePathNode / widePathSlot [g][j].  Every other phase runs the single-playout code on the
// slot's first row.
static_assert(sizeof(DBoard) % 4 == 0, "DBoard copy granularity");
KC_D void saveLeaf(const GV& v, const GameDev& s, WideRec* r) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&s.leaf);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&r->leaf);
  for(int i = v.lane; i < (int)(sizeof(DBoard) / 4); i += 64)
    dst[i] = src[i];
  if(v.lane == 0) {
    r->leafKind = s.leafKind;
    r->leafNode = s.leafNode;
    r->leafSym = s.leafSym;
    r->nnSlot = s.nnSlot;
    r->cSlot = s.cSlot;
    r->pathLen = s.pathLen;
    r->cHitWin = s.cHitWin;
    r->cHitLoss = s.cHitLoss;
    r->cHitErr = s.cHitErr;
  }
}
KC_D void loadLeaf(const GV& v, GameDev& s, const WideRec* r) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&r->leaf);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&s.leaf);
  for(int i = v.lane; i < (int)(sizeof(DBoard) / 4); i += 64)
    dst[i] = src[i];
  s.leafKind = r->leafKind;
  s.leafNode = r->leafNode;
  s.leafSym = r->leafSym;
  s.nnSlot = r->nnSlot;
  s.cSlot = r->cSlot;
  s.pathLen = r->pathLen;
  s.cHitWin = r->cHitWin;
  s.cHitLoss = r->cHitLoss;
  s.cHitErr = r->cHitErr;
  waveSync();
}

template <int NI, bool EXPL = false>
__global__ void __launch_bounds__(64, NI <= 2 ? 4 : 2) kSelectWide(const SearchDev* __restrict__ dp,
                                                                    const DTables* __restrict__ Tp, int resetCommit) {
  const SearchDev& d = *dp;
  const int g = blockIdx.x;
  if(resetCommit && g == 0 && threadIdx.x == 0)
    *d.commitCount = 0;
  if(g >= d.G)
    return;
  __shared__ uint32_t hasBits[(MAX_P + 31) / 32];
  __shared__ GameDev s;
  __shared__ float rootPol[MAX_P];
  const int K = d.wideK, lane = laneId();
  if(lane < K)
    d.nnNeed[g * K + lane] = 0;
  const int phase = __builtin_amdgcn_readfirstlane(d.games[g].phase);
  if(phase != PH_SEARCH) {
    if(lane == 0)
      d.wideCount[g] = 0;
    if(phase == PH_COMMIT) {  // idle, or waiting for its report
      if(lane == 0)
        d.games[g].leafKind = LEAF_NONE;
      return;
    }
    selectBody<NI, false, EXPL>(d, *Tp, g, s, false, false, hasBits, rootPol, g * K);
    return;
  }
  GV v(d, *Tp, g);
  loadGame(v, s);
  DRng rng = DRng{s.rngSeed, s.rngCtr};
  // never past the visit limit: every descent that does not collide adds one root visit
  const int left = s.visitLimit - (int)v.nodes()[s.rootIdx].visits;
  const int n = left < K ? left : K;
  int made = 0;
  bool collided = false;
  for(int j = 0; j < n && !collided; j++) {
    v.setDescent(j);
    descend<NI, EXPL, true>(v, s, hasBits, rootPol, j == 0);
    made = j + 1;
    collided = s.leafKind == LEAF_COLLISION;
    if(collided) {
      removeVirtualLosses(v, s.pathLen, s.leafNode);
    } else {
      if(s.leafKind == LEAF_NN && d.cacheOn)
        cacheLookup<NI>(v, s, false);
      finishLeaf<W1_OF<NI>>(v, s, rng);
    }
    waveSync();
    saveLeaf(v, s, d.wideRec + v.row);
    waveSync();
  }
  s.leafKind = LEAF_WIDE;
  if(lane == 0) {
    d.wideCount[g] = made;
    atomicAdd(&d.wideCtr[WC_DESCENTS], (unsigned long long)made);
    if(collided)
      atomicAdd(&d.wideCtr[WC_COLLISIONS], 1ull);
  }
  waveSync();
  storeGame(v, s);
}

template <int NI, bool EXPL = false>
__global__ void __launch_bounds__(64, NI <= 4 ? 4 : 3) kBackupWide(const SearchDev* __restrict__ dp,
                                                                    const DTables* __restrict__ Tp) {
  const SearchDev& d = *uniformConst(dp);  // constant views: see kBackup
  const DTables& T = *uniformConst(Tp);
  const int g = blockIdx.x;
  if(g >= d.G)
    return;
  __shared__ __attribute__((aligned(16))) float scratch[3 * MAX_P];
  __shared__ GameDev s;
  if(__builtin_amdgcn_readfirstlane(d.games[g].leafKind) != LEAF_WIDE) {
    backupBody<NI, false, EXPL, true>(d, T, g, s, false, scratch);
    return;
  }
  GV v(d, T, g);
  loadGame(v, s);
  const int made = __builtin_amdgcn_readfirstlane(d.wideCount[g]);
  for(int j = 0; j < made; j++) {
    v.setDescent(j);
    loadLeaf(v, s, d.wideRec + v.row);
    if(s.leafKind == LEAF_COLLISION)  // the round's last: its virtual losses came off in the selection
      break;
    playoutBackup<NI, false, EXPL>(v, s, d.P, d.nnOut + (size_t)s.nnSlot * (d.P + 4), false, scratch);
    removeVirtualLosses(v, s.pathLen, s.leafNode);
  }
  // the commit test once, after the last backup
  if(v.nodes()[s.rootIdx].visits >= (uint32_t)s.visitLimit) {
    s.phase = PH_COMMIT;
    if(v.lane == 0)
      d.commitList[atomicAdd(d.commitCount, 1)] = g;
  }
  s.leafKind = LEAF_NONE;
  waveSync();
  storeGame(v, s);
}

// The batch of a wide round: the rows that need the network in ascending order, and each one's bid
// for its NN-cache slot (the highest row stores, as the highest game does in kCompact).  One
// workgroup; a wide engine's rows never exceed its batch cap (coffee_analysis_set_search_threads),
// so no row is deferred.
__global__ void __launch_bounds__(1024) kCompactWide(const SearchDev* __restrict__ dp, int accumulate) {
  const SearchDev& d = *dp;
  __shared__ int wsum[16];
  const int nt = blockDim.x, nw = nt >> 6;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int R = d.G * d.wideK;
  const uint64_t below = (1ull << lane) - 1ull;
  int base = 0;  // rows listed by the chunks before (uniform)
  for(int c0 = 0; c0 < R; c0 += nt) {
    const int i = c0 + t;
    const bool nd = i < R && d.nnNeed[i] != 0;
    const uint64_t b = ballot(nd);
    if(lane == 0)
      wsum[w] = __popcll(b);
    __syncthreads();
    int off = base, tot = 0;
    for(int q = 0; q < nw; q++) {
      off += q < w ? wsum[q] : 0;
      tot += wsum[q];
    }
    if(nd) {
      d.nnIdx[off + __popcll(b & below)] = i;
      const uint32_t bid = d.nnBid[i];
      if(bid != ~0u)
        atomicMax(&d.cTag[bid], (uint32_t)i + 1u);
    }
    base += tot;
    __syncthreads();
  }
  if(t == 0) {
    *d.nnCount = base;
    *d.pendCount = 0;
    if(accumulate)
      *d.nnTimedEvals += (unsigned long long)base;
  }
}

// The virtual losses live in the engine's trees (0 between rounds): one wave per slot over the
// slot's allocated nodes.
__global__ void __launch_bounds__(64) kVirtualLossCount(const SearchDev* __restrict__ dp, unsigned long long* out) {
  const SearchDev& d = *dp;
  const int g = blockIdx.x, lane = laneId();
  const Node* NS = d.nodes + (size_t)g * d.cap;
  const uint32_t* bits = d.allocBits + (size_t)g * (d.cap / 32);
  int sum = 0;
  for(int i = lane; i < d.cap; i += 64)
    if((bits[i >> 5] >> (i & 31)) & 1u)
      sum += NS[i].virtualLosses;
#pragma unroll
  for(int off = 32; off >= 1; off >>= 1)
    sum += __shfl_xor(sum, off, 64);
  if(lane == 0 && sum != 0)
    atomicAdd(out, (unsigned long long)sum);
}

#ifdef KC_SEARCH_PROFILE
}  // namespace kc
#include <algorithm>
#include <vector>
namespace kc {
extern "C" void coffee_debug_probe_table(void* keys, unsigned long long cap /* power of two */) {
  unsigned long long* k = (unsigned long long*)keys;
  unsigned long long m = cap ? cap - 1 : 0;
  KC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_probeKeys), &k, sizeof(k)));
  KC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_probeMask), &m, sizeof(m)));
}

extern "C" void coffee_debug_search_profile(unsigned long long* out, int reset) {
  std::vector<unsigned long long> all((size_t)SPROF_MAXG * SPROF_N);
  KC_HIP(hipDeviceSynchronize());
  KC_HIP(hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_searchProf), all.size() * 8));
  for(int i = 0; i < SPROF_N; i++)
    out[i] = 0;
  for(size_t k = 0; k < all.size(); k++) {
    const int i = (int)(k % SPROF_N);
    if(i < 24 || i >= 32)
      out[i] += all[k];
    else if(i <= 26)
      out[i] = std::max(out[i], all[k]);
    if(i == 24)
      out[27] += all[k];  // sum of per-block maxima (their mean: the typical slowest descent)
    if(i == 26)
      out[28] += all[k];
  }
  if(reset) {
    std::fill(all.begin(), all.end(), 0ull);
    KC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_searchProf), all.data(), all.size() * 8));
  }
}
#endif

// ---------------------------------------------------------------------------
// Commit: move choice, targets, tree reuse, rows.

// oracle lcbAndRadius (getSelfUtilityLCBAndRadius searchhelpers.cpp:469-521)
KC_D void lcbAndRadius(const SP& sp, int pla, uint32_t cVisits, float cWs, float cWsq, float cU, float cUsq,
                       uint32_t ev, float& lcb, float& radius) {
  radius = 2.0f * 1.0f * sp.lcbStdevs;
  lcb = -radius;
  float ws = childWeight(ev, cVisits, cWs);
  float wsq = childWeight(ev, cVisits, cWsq);
  if(cVisits == 0 || ws <= 0.0f || wsq <= 0.0f)
    return;
  float u = cU, usq = cUsq;
  float ess = (ws * ws) / wsq;
  float priorWeight = ws / ((ess * ess) * ess);
  usq = fmaxf(usq, u * u + 1e-8f);
  usq = (usq * ws + (usq + 1.0f) * priorWeight) / (ws + priorWeight);
  ws = ws + priorWeight;
  wsq = wsq + priorWeight * priorWeight;
  ess = (ws * ws) / wsq;
  float selfU = pla == 2 ? u : -u;
  float variance = usq - u * u;
  float stdev = sqrtf(variance / ess);
  radius = stdev * sp.lcbStdevs;
  lcb = selfU - radius;
}

// oracle playSelectionValuesAt (getPlaySelectionValues searchresults.cpp:63-309) on node
// ri with policy pol; the over-explored-children reduction and direct policy moves are
// root-only.  posOut/vals are LDS arrays [P]; returns the count (uniform).
template <int NI, bool EXPL = false>
KC_D int playSelectionValuesAt(const GV& v, const SP& sp, const GameDev& s, int ri, const float* pol, bool isRoot,
                               float scaleMaxToAtLeast, bool allowDirect, int* posOut, float* vals, bool useLcb) {
  const Node& n = v.nodes()[ri];
  const int k = n.numChildren;
  const int pla = n.nextPla;
  const NodeEdges E = v.edges(ri, n.edgeBase);
  float cw[NI], val[NI];
  uint32_t ev[NI];
  int posv[NI];
  uint32_t cvis[NI];
  float cws[NI], cwsq[NI], cu[NI], cusq[NI];
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = v.lane + 64 * j;
    cw[j] = val[j] = 0.0f;
    ev[j] = 0;
    posv[j] = 0;
    cvis[j] = 0;
    cws[j] = cwsq[j] = cu[j] = cusq[j] = 0.0f;
    if(i < k) {
      Edge e = E[i];
      const Node& c = v.nodes()[e.child];
      cvis[j] = c.visits;
      cws[j] = c.weightSum;
      cwsq[j] = c.weightSqSum;
      cu[j] = c.utilityAvg;
      cusq[j] = c.utilitySqAvg;
      ev[j] = e.visits;
      cw[j] = childWeight(e.visits, cvis[j], cws[j]);
      posv[j] = (int)e.move;
      val[j] = cw[j];
    }
  }
  const float total = tsum<NI>(cw, k, v.lane);
  int numChildren = k;
  // best child by "good" weight (first max)
  float maxGood = -1e30f;
  int bestIdx = BIG;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = v.lane + 64 * j;
    if(i >= k)
      continue;
    float evf = (float)ev[j];
    float gdn = val[j] * fmaxf(0.0f, evf - 1.0f) / fmaxf(1.0f, evf) + 2.0f * pol[posv[j]];
    if(gdn > maxGood) {
      maxGood = gdn;
      bestIdx = i;
    }
  }
  waveArgmax(maxGood, bestIdx);
  if(bestIdx == BIG)
    bestIdx = 0;
  const int bestLane = bestIdx & 63, bestJ = bestIdx >> 6;
  float bestWeight = -1e30f;
  if(k > 0) {
    float bw = 0.0f;
#pragma unroll
    for(int j = 0; j < NI; j++)
      if(j == bestJ)
        bw = cw[j];
    bestWeight = bcastLaneF(bw, bestLane);
  }
  if(isRoot && k > 0) {
    const float fpu = fpuValue(sp, n, pla, true, 1.0f);
    float scaling = exploreScaling(sp, total);
    if constexpr(EXPL)
      scaling = scaling * exploreStdevFactor(explOf(v), n.visits, n.weightSum, n.utilityAvg, n.utilitySqAvg);
    float bp = 0.0f, bu = 0.0f;
    uint32_t bvis = 0;
#pragma unroll
    for(int j = 0; j < NI; j++)
      if(j == bestJ) {
        bp = pol[posv[j]];
        bu = cu[j];
        bvis = cvis[j];
      }
    bp = bcastLaneF(bp, bestLane);
    bu = bcastLaneF(bu, bestLane);
    bvis = (uint32_t)bcastLane((int)bvis, bestLane);
    const float bw = bestWeight;
    const float buu = (bvis == 0 || bw <= 0.0f) ? fpu : bu;
    const float bestValue = bp < 0.0f ? -__builtin_inff() : (scaling * bp) / (1.0f + bw) + (pla == 2 ? buu : -buu);
#pragma unroll
    for(int j = 0; j < NI; j++) {
      int i = v.lane + 64 * j;
      if(i >= k || i == bestIdx)
        continue;
      float w = cw[j];
      float reduced;
      if(cvis[j] == 0 || w <= 0.0f)
        reduced = 0.0f;
      else {
        float p = pol[posv[j]];
        float wanted;
        if(p < 0.0f)
          wanted = 0.0f;
        else {
          float valueComponent = pla == 2 ? cu[j] : -cu[j];
          float exploreComponent = bestValue - valueComponent;
          float exploreComponentScaling = scaling * p;
          if(exploreComponent <= 0.0f)
            wanted = __builtin_inff();
          else {
            wanted = exploreComponentScaling / exploreComponent - 1.0f;
            if(wanted < 0.0f)
              wanted = 0.0f;
          }
        }
        reduced = w > wanted ? wanted : w;
      }
      val[j] = ceilf(reduced);
    }
  }
  if(useLcb && k > 0) {
    float lcb[NI], rad[NI];
    float bestLcb = -1e10f;
    int bestLcbIdx = BIG;
#pragma unroll
    for(int j = 0; j < NI; j++) {
      int i = v.lane + 64 * j;
      lcb[j] = rad[j] = 0.0f;
      if(i >= k)
        continue;
      lcbAndRadius(sp, pla, cvis[j], cws[j], cwsq[j], cu[j], cusq[j], ev[j], lcb[j], rad[j]);
      float w = val[j];
      if(w > 0.0f && w >= sp.minVisitPropLcb * bestWeight && lcb[j] > bestLcb) {
        bestLcb = lcb[j];
        bestLcbIdx = i;
      }
    }
    waveArgmax(bestLcb, bestLcbIdx);
    if(bestLcbIdx != BIG) {
      float adj = 0.0f;
#pragma unroll
      for(int j = 0; j < NI; j++)
        if(j == (bestLcbIdx >> 6))
          adj = val[j];
      adj = bcastLaneF(adj, bestLcbIdx & 63);
      float lb = adj;
#pragma unroll
      for(int j = 0; j < NI; j++) {
        int i = v.lane + 64 * j;
        if(i >= k || i == bestLcbIdx)
          continue;
        float excess = bestLcb - lcb[j];
        if(excess < 0.0f)
          continue;
        float rf = (rad[j] + excess) / (rad[j] + 0.20f * excess);
        float lbound = (rf * rf) * val[j];
        if(lbound > lb)
          lb = lbound;
      }
      lb = waveMax(lb);
#pragma unroll
      for(int j = 0; j < NI; j++)
        if(v.lane + 64 * j == bestLcbIdx)
          val[j] = lb;
    }
  }
  // to LDS
#pragma unroll
  for(int j = 0; j < NI; j++) {
    int i = v.lane + 64 * j;
    if(i < k) {
      posOut[i] = posv[j];
      vals[i] = val[j];
    }
  }
  waveSync();
  if(numChildren == 0) {
    if(!allowDirect || !isRoot)
      return 0;
    const int P = v.d.P;
    for(int base = 0; base < P; base += 64) {
      int p = base + v.lane;
      bool ok = p < P && isLegal(v.T, s.root, p % v.T.A, p / v.T.A) && pol[p] >= 0.0f;
      uint64_t m = ballot(ok);
      if(ok) {
        int idx = numChildren + __popcll(m & ((1ULL << v.lane) - 1ULL));
        posOut[idx] = p;
        vals[idx] = pol[p];
      }
      numChildren += __popcll(m);
    }
    waveSync();
    if(numChildren == 0)
      return 0;
  }
  float mx = 0.0f;
  for(int i = v.lane; i < numChildren; i += 64)
    mx = vals[i] > mx ? vals[i] : mx;
  mx = waveMax(mx);
  if(mx <= 0.0f)
    return 0;
  const float amountToSubtract = fminf(sp.moveSubtract, mx / 64.0f);
  const float amountToPrune = fminf(sp.movePrune, mx / 64.0f);
  const float newMax = mx - amountToSubtract;
  for(int i = v.lane; i < numChildren; i += 64) {
    float x = vals[i];
    if(x < amountToPrune)
      x = 0.0f;
    else {
      x = x - amountToSubtract;
      if(x <= 0.0f)
        x = 0.0f;
    }
    if(newMax < scaleMaxToAtLeast)
      x = x * (scaleMaxToAtLeast / newMax);
    vals[i] = x;
  }
  waveSync();
  return numChildren;
}

// oracle playSelectionValues: the root with its noised policy.
template <int NI, bool EXPL = false>
KC_D int playSelectionValues(const GV& v, const SP& sp, const GameDev& s, float scaleMaxToAtLeast, bool allowDirect,
                             int* posOut, float* vals, bool useLcb) {
  return playSelectionValuesAt<NI, EXPL>(v, sp, s, s.rootIdx, v.rootNoised(), true, scaleMaxToAtLeast, allowDirect, posOut,
                                   vals, useLcb);
}

// oracle chooseIndex (chooseIndexWithTemperature searchhelpers.cpp:11-49)
KC_D int chooseIndex(const GV& v, DRng& rng, const float* vals, int n, float temperature, float* pr) {
  float mx = 0.0f;
  for(int i = v.lane; i < n; i += 64)
    mx = vals[i] > mx ? vals[i] : mx;
  mx = waveMax(mx);
  if(temperature <= 1.0e-4f) {
    float best = -__builtin_inff();
    int bi = BIG;
    for(int i = v.lane; i < n; i += 64)
      if(vals[i] > best) {
        best = vals[i];
        bi = i;
      }
    waveArgmax(best, bi);
    // oracle: best starts at vals[0]; strictly greater later values win
    return bi == BIG ? 0 : bi;
  }
  const float logMax = dlog(mx);
  for(int i = v.lane; i < n; i += 64)
    pr[i] = vals[i] <= 0.0f ? 0.0f : dexp((dlog(vals[i]) - logMax) / temperature);
  const float sum = seqSum(pr, n, v.lane);
  const float dd = rng.uni() * sum;
  int chosen = n - 1;
  if(v.lane == 0) {
    float acc = 0.0f;
    for(int i = 0; i < n; i++) {
      acc = acc + pr[i];
      if(acc > dd) {
        chosen = i;
        break;
      }
    }
  }
  return bcastI(chosen, 0);
}

// 16-byte stores where the arrays allow (every per-game slice starts 16-B aligned when
// its length is a multiple of 4 words), one word at a time otherwise.
KC_D void fillWords(uint32_t* p, int n, uint32_t val, int lane) {
  if((n & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    uint4* q = reinterpret_cast<uint4*>(p);
    for(int i = lane; i < n / 4; i += 64)
      q[i] = uint4{val, val, val, val};
  } else {
    for(int i = lane; i < n; i += 64)
      p[i] = val;
  }
}

KC_D void clearTables(const GV& v, GameDev& s) {
  const int cap = v.d.cap;
  uint32_t* fl = v.freeList();
  if((cap & 3) == 0 && (reinterpret_cast<uintptr_t>(fl) & 15) == 0) {
    uint4* q = reinterpret_cast<uint4*>(fl);
    for(int i = v.lane; i < cap / 4; i += 64) {
      const uint32_t b = (uint32_t)(cap - 1 - 4 * i);  // pop order: 0, 1, 2, ...
      q[i] = uint4{b, b - 1, b - 2, b - 3};
    }
  } else {
    for(int i = v.lane; i < cap; i += 64)
      fl[i] = (uint32_t)(cap - 1 - i);
  }
  fillWords(v.allocBits(), cap / 32, 0u, v.lane);
  fillWords(reinterpret_cast<uint32_t*>(v.ttNode()), v.d.ttCap, 0xFFFFFFFFu, v.lane);
  const size_t sb = v.svbBase(s.svbSel);
  fillWords(reinterpret_cast<uint32_t*>(&v.d.svbKey[sb]), 2 * v.d.svbCap, 0u, v.lane);
  s.freeTop = cap;
  s.edgeTop = 0;
  s.liveCount = 0;
  s.rootIdx = -1;
  waveSync();
}

// oracle reuseTree (Search::makeMove search.cpp:262-330 + deleteAllOld... :790-810 +
// SubtreeValueBiasTable::clearUnusedSynchronous :47-59) as mark / free / rebuild.
// lds: live bitmap [cap/32] u32 + BFS queue [cap] u16.
KC_D void reuseTree(const GV& v, GameDev& s, int chosenPos, uint32_t* liveBits, uint16_t* queue, int* qtail) {
  const SP& sp = *v.sp;
  const int cap = v.d.cap;
  const int ri = s.rootIdx;
  int child = -1;
  if(ri >= 0) {
    const Node& r = v.nodes()[ri];
    const NodeEdges E = v.edges(ri, r.edgeBase);
    for(int base = 0; base < r.numChildren; base += 64) {
      int i = base + v.lane;
      bool hit = i < r.numChildren && (int)E[i].move == chosenPos;
      uint64_t m = ballot(hit);
      if(m) {
        int f = firstLane(m);
        child = bcastI(hit ? (int)E[i].child : -1, f);
        break;
      }
    }
  }
  if(child < 0 || !(v.nodes()[child].flags & 1)) {
    clearTables(v, s);
    return;
  }
  // mark: parallel BFS over child slots
  for(int i = v.lane; i < cap / 32; i += 64)
    liveBits[i] = 0;
  waveSync();
  if(v.lane == 0) {
    liveBits[child >> 5] |= 1u << (child & 31);
    queue[0] = (uint16_t)child;
    *qtail = 1;
  }
  waveSync();
  int head = 0;
  while(true) {
    const int tail = *qtail;
    if(head >= tail)
      break;
    const int cnt = min(64, tail - head);
    if(v.lane < cnt) {
      const int nd = queue[head + v.lane];
      const Node& nr = v.nodes()[nd];
      const int kc = nr.numChildren;
      const Edge* inl = v.inlineEdges(nd);
      const Edge* pool = v.edgePool() + nr.edgeBase - INLINE_EDGES;  // indexed by child slot
      // four child loads in flight before the LDS atomics that consume them
      for(int i = 0; i < kc; i += 4) {
        int ch[4];
#pragma unroll
        for(int u = 0; u < 4; u++)
          ch[u] = i + u < kc ? (int)(i + u < INLINE_EDGES ? inl : pool)[i + u].child : -1;
#pragma unroll
        for(int u = 0; u < 4; u++) {
          const int c = ch[u];
          if(c < 0)
            continue;
          const uint32_t bit = 1u << (c & 31);
          uint32_t old = atomicOr(&liveBits[c >> 5], bit);
          if(!(old & bit))
            queue[atomicAdd(qtail, 1)] = (uint16_t)c;
        }
      }
    }
    head += cnt;
    waveSync();
  }
  int liveCount = 0;
  for(int i = v.lane; i < cap / 32; i += 64)
    liveCount += __popc(liveBits[i]);
#pragma unroll
  for(int off = 32; off >= 1; off >>= 1)
    liveCount += __shfl_xor(liveCount, off, 64);
  if(liveCount + sp.maxVisits + 2 > cap) {
    clearTables(v, s);
    return;
  }
  // removeSubtreeValueBias for dead table nodes and the promoted child (fixed point: any order).
  // The dead allocated nodes are compacted into the queue behind the live ones
  // (queue[0..liveCount) = live nodes in BFS order; dead <= cap - liveCount), so the
  // node reads below are independent and batched; lane 0 adds the child.
  const size_t sb = v.svbBase(s.svbSel);
  uint32_t* ab = v.allocBits();
  const int nw = cap / 32;
  uint16_t* dead = queue + liveCount;
  int nDead = 0;
  for(int wb = 0; wb < nw; wb += 64) {
    const int w = wb + v.lane;
    uint32_t m = 0;
    if(w < nw)
      m = ab[w] & ~liveBits[w];
    int cnt = __popc(m), incl = cnt;
#pragma unroll
    for(int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(incl, off, 64);
      if(v.lane >= off)
        incl += y;
    }
    int o = nDead + incl - cnt;
    while(m) {
      const int b = __builtin_ctz(m);
      m &= m - 1;
      dead[o++] = (uint16_t)(w * 32 + b);
    }
    nDead += __shfl(incl, 63, 64);
  }
  waveSync();
  for(int base = 0; base < nDead + 1; base += 256) {
    int32_t e[4];
    float dl[4], wl[4];
#pragma unroll
    for(int u = 0; u < 4; u++) {
      const int i = base + 64 * u + v.lane;  // i == nDead: the promoted child
      e[u] = -1;
      dl[u] = wl[u] = 0.0f;
      if(i <= nDead) {
        const Node& n = v.nodes()[i < nDead ? (int)dead[i] : child];
        e[u] = n.svbEntry;
        dl[u] = n.lastSvbDelta;
        wl[u] = n.lastSvbWeight;
      }
    }
#pragma unroll
    for(int u = 0; u < 4; u++) {
      if(e[u] < 0)
        continue;
      atomicAdd((unsigned long long*)&v.d.svbD[sb + e[u]], (unsigned long long)(-svbQ(dl[u] * sp.svbFreeProp)));
      atomicAdd((unsigned long long*)&v.d.svbW[sb + e[u]], (unsigned long long)(-svbQ(wl[u] * sp.svbFreeProp)));
    }
  }
  waveSync();
  if(v.lane == 0) {
    Node* c = &v.nodes()[child];
    c->svbEntry = -1;
    c->lastSvbDelta = 0.0f;
    c->lastSvbWeight = 0.0f;
  }
  // free list = every non-live index; allocBits = live
  int top = 0;
  uint32_t* fl = v.freeList();
  for(int base = 0; base < cap; base += 64) {
    int i = base + v.lane;
    bool live = (liveBits[i >> 5] >> (i & 31)) & 1u;
    uint64_t m = ballot(!live);
    if(!live)
      fl[top + __popcll(m & ((1ULL << v.lane) - 1ULL))] = (uint32_t)i;
    top += __popcll(m);
  }
  for(int i = v.lane; i < cap / 32; i += 64)
    ab[i] = liveBits[i];
  s.freeTop = top;
  s.liveCount = liveCount;
  s.rootIdx = child;
  // transposition table: clear, insert every live node but the root (CAS, any order)
  int32_t* tn = v.ttNode();
  uint64_t* tk = v.ttKey();
  for(int i = v.lane; i < v.d.ttCap; i += 64)
    tn[i] = -1;
  // new SVB table
  const int nsel = s.svbSel ^ 1;
  const size_t nb = v.svbBase(nsel);
  for(int i = v.lane; i < v.d.svbCap; i += 64)
    v.d.svbKey[nb + i] = 0;
  waveSync();
  const int tmask = v.d.ttCap - 1, smask = v.d.svbCap - 1;
  // live nodes, in the order of the BFS queue (queue[0..liveCount) holds them all)
  for(int i = v.lane; i < liveCount; i += 64) {
    const int ni = queue[i];
    Node* n = &v.nodes()[ni];
    const int32_t se = n->svbEntry;
    if(ni != child && v.d.sp.useGraph) {
      const uint64_t k0 = v.nodeKey(ni)[0], k1 = v.nodeKey(ni)[1];
      int sl = (int)(k0 & (uint64_t)tmask);
      while(atomicCAS(&tn[sl], -1, ni) != -1)
        sl = (sl + 1) & tmask;
      tk[2 * sl] = k0;
      tk[2 * sl + 1] = k1;
    }
    if(se >= 0) {
      const size_t oe = sb + se;
      const uint64_t key = v.d.svbKey[oe];
      int sl = (int)(key & (uint64_t)smask);
      while(true) {
        unsigned long long prev =
          atomicCAS((unsigned long long*)&v.d.svbKey[nb + sl], 0ULL, (unsigned long long)key);
        if(prev == 0ULL || prev == key)
          break;
        sl = (sl + 1) & smask;
      }
      v.d.svbD[nb + sl] = v.d.svbD[oe];
      v.d.svbW[nb + sl] = v.d.svbW[oe];
      n->svbEntry = sl;
    }
  }
  s.svbSel = nsel;
  // edge pool: the live nodes' blocks into the other buffer (queue order, prefix sums
  // of the block sizes), so the dead nodes' blocks are reclaimed
  {
    const int P = v.d.P;
    Edge* src = v.edgePool();
    Edge* dst = v.d.edgePool + ((size_t)v.g * 2 + (s.edgeSel ^ 1)) * v.d.edgePoolCap;
    int top = 0;
    for(int base = 0; base < liveCount; base += 64) {
      const int i = base + v.lane;
      const int nd = i < liveCount ? (int)queue[i] : -1;
      const Node* np = nd >= 0 ? &v.nodes()[nd] : nullptr;
      const int k = np ? (int)np->numChildren : 0;
      const int need = k > INLINE_EDGES ? edgeBlockCap(k, P) : 0;
      int incl = need;
#pragma unroll
      for(int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off, 64);
        if(v.lane >= off)
          incl += y;
      }
      const int mine = top + incl - need;
      if(need) {
        const uint32_t ob = np->edgeBase;
        for(int e = 0; e < k - INLINE_EDGES; e++)
          dst[mine + e] = src[ob + e];
        v.nodes()[nd].edgeBase = (uint32_t)mine;
      }
      top += __shfl(incl, 63, 64);
    }
    const int nsel2 = s.edgeSel ^ 1;
    waveSync();
    s.edgeSel = nsel2;
    s.edgeTop = top;
    s.edgePeak = max(s.edgePeak, top);
    v.setEdgeSel(nsel2);
  }
  waveSync();
}

// oracle setMoveLimits (getSearchLimitsThisMove play.cpp:871-1004) for the move about
// to be searched; every lane runs it on the same state.  lastWL: the root value of the
// move just committed (the newest reduceVisits history entry).  Returns
// clearBotBeforeSearchThisMove (self-play clears before every search, play.cpp:1941-1946,
// except a cheap search whose rows are not recorded, :920-925).
KC_D bool setMoveLimits(const GV& v, GameDev& s, DRng& rng, float lastWL) {
  const SP& b = v.d.sp;
  s.visitLimit = b.maxVisits;
  s.moveWeight = 1.0f;
  s.noNoise = 0;
  bool clear = true;
  if(b.cheapProb > 0.0f && rng.uni() < b.cheapProb) {
    s.visitLimit = min(b.maxVisits, b.cheapVisits);
    s.moveWeight = 1.0f * b.cheapWeight;
    if(b.cheapWeight <= 0.0f) {
      clear = false;
      s.noNoise = 1;
    }
  } else if(b.reduceVisits && s.numTurns - s.startTurn >= b.reduceLookback) {
    const TurnRec* tr = v.turns();
    float mn = 1e20f, mx = -1e20f;
    for(int j = 0; j < b.reduceLookback; j++) {
      const float w = j == 0 ? lastWL : tr[s.numTurns - 1 - j].rootWL;
      mn = w < mn ? w : mn;
      mx = w > mx ? w : mx;
    }
    float extreme = fmaxf(mn, -mx);
    if(extreme > 1.0f)
      extreme = 1.0f;
    const float through = extreme - b.reduceThreshold;
    if(through > 0.0f) {
      const float prop = through / (1.0f - b.reduceThreshold);
      const float red = prop * prop;
      const int vl = (int)roundf((float)b.maxVisits + red * ((float)b.reducedMin - (float)b.maxVisits));
      s.moveWeight = 1.0f + red * (b.reducedWeight - 1.0f);
      s.visitLimit = max(vl, b.reducedMin);
    }
  }
  return clear;
}

// The replay of start-position sample `sp` from the empty board into b (every lane holds the
// same b; the rules are wave-wide).  Every decision is taken on readfirstlane values, so the
// branches stay scalar and every lane stays active for playMoveWave's ballot.
// CHECK: each move is tested before it is played and the index of the first bad one returned
// (-1: none); without it the moves are only clamped into the policy range -- the table passed
// the check before it was set -- and the replay stops should the game end.  nm: the moves
// played.  Nothing indexes past the sample or the tables whatever the sample holds.
template <bool W1, bool CHECK>
KC_D int replayStartPos(const DTables& T, DBoard& b, const coffee_start_position* sp, int A, int P, int& nm) {
  const int want = __builtin_amdgcn_readfirstlane((int)sp->num_moves);
  const int n = min(max(want, 0), min(A - 1, COFFEE_ANALYSIS_MAX_MOVES));
  boardInit(T, b);
  waveSync();
  int bad = -1, t = 0;
  for(; t < n; t++) {
    int mv = __builtin_amdgcn_readfirstlane((int)sp->moves[t]);
    if(__builtin_amdgcn_readfirstlane(b.finished) != 0) {
      bad = t;
      break;
    }
    if(CHECK) {
      bool ok = mv < P;
      if(ok)
        ok = __builtin_amdgcn_readfirstlane((int)isLegal<W1>(T, b, mv % A, mv / A)) != 0;
      if(!ok) {
        bad = t;
        break;
      }
    } else {
      mv = min(mv, P - 1);
    }
    playMoveWave<W1>(T, b, mv % A, mv / A);
    waveSync();
  }
  nm = t;
  return bad;
}

// One wave per sample of a start-position table: the replay with the device rules, status and
// info as analysisRefill reports a query it cannot search.
template <int NI>
__global__ void __launch_bounds__(64) kStartPosCheck(const DTables* __restrict__ Tp,
                                                     const coffee_start_position* __restrict__ samples, int n,
                                                     int32_t* __restrict__ status, int32_t* __restrict__ info) {
  const DTables& T = *Tp;
  const int i = blockIdx.x;
  if(i >= n)
    return;
  __shared__ DBoard b;
  const coffee_start_position* sp = samples + i;
  const int A = T.A, P = T.P;
  const int want = __builtin_amdgcn_readfirstlane((int)sp->num_moves);
  int nm = 0;
  const int bad = replayStartPos<W1_OF<NI>, true>(T, b, sp, A, P, nm);
  waveSync();
  int st = COFFEE_ANALYSIS_OK, inf = 0;
  if(want < 0 || want >= A || want > COFFEE_ANALYSIS_MAX_MOVES) {
    st = COFFEE_ANALYSIS_ILLEGAL_MOVE;
    inf = -1;
  } else if(bad >= 0) {
    st = COFFEE_ANALYSIS_ILLEGAL_MOVE;
    inf = bad;
  } else if(b.finished != 0) {
    if(b.winner == 0 && b.turn < A) {
      st = COFFEE_ANALYSIS_NO_LEGAL_MOVE;
    } else {
      st = COFFEE_ANALYSIS_GAME_OVER;
      inf = b.winner;
    }
  }
  if(laneId() == 0) {
    status[i] = st;
    info[i] = inf;
  }
}

// The moves of start-position sample sp as unsearched turn records of game v.g (as
// startForkGame and analysisRefill write theirs); nm: the moves the replay played.
KC_D void writeStartPosTurns(const GV& v, const coffee_start_position* sp, int nm) {
  TurnRec* tr = v.turns();
  for(int t = v.lane; t < nm; t += 64) {
    const int mv = min((int)sp->moves[t], v.T.P - 1);
    TurnRec rec;
    memset(&rec, 0, sizeof(rec));
    rec.gen = (uint8_t)*v.d.modelGen;
    rec.cell = (int8_t)(mv % v.T.A);
    rec.dir = (int8_t)(mv / v.T.A);
    tr[t] = rec;
  }
}

// deferTurns (kCommit): a start position's turn records are left to kStartPosTurns, which
// runs after kRows -- that kernel still reads the finished game's records from the same array.
KC_D void startGame(const GV& v, GameDev& s, bool deferTurns) {
  s.rngSeed = gameStreamSeed(v.d.seed, (uint32_t)(v.d.slotBase + v.g), (uint32_t)s.gameNum);
  s.rngCtr = 0;
  s.startGen = *v.d.modelGen;
  boardInit(v.T, s.root);
  clearTables(v, s);
  s.numTurns = 0;
  s.gameMode = 0;
  s.sideCount = 0;
  s.sideNext = 0;
  s.sideMode = 0;
  DRng rng{s.rngSeed, s.rngCtr};
  s.gameHash0 = rng.next();
  s.gameHash1 = rng.next();
  // initializeGameUsingPolicy (playutils.cpp:147-176): floor(Exp(1) * area * prop)
  // opening moves sampled from the raw policy (nextExponential rand.h:299-305)
  s.startTurn = 0;
  s.initLeft = 0;
  s.spPending = 0;
  const SP& b = v.d.sp;
  float areaProp = b.initAreaProp;
  // start positions (startpos.h; play.cpp:400-448): with a table set, a share of the games
  // starts from a sampled move list, replayed here as unsearched turns; policy init stays
  // allowed with its own area proportion (allowPolicyInit, play.cpp:1228-1231).  No table or
  // probability 0: no draw
  const int spN = __builtin_amdgcn_readfirstlane(v.d.spN);
  if(spN > 0) {
    const uint64_t* cum = v.d.spCum;
    const int pick = __builtin_amdgcn_readfirstlane(startPosDraw(rng, v.d.spProb, cum, spN));
    if(pick >= 0) {
      const coffee_start_position* sp = v.d.spTable + min(pick, spN - 1);
      int nm = 0;
      replayStartPos<false, false>(v.T, s.root, sp, v.T.A, v.T.P, nm);
      nm = __builtin_amdgcn_readfirstlane(nm);
      if(deferTurns)
        s.spPending = min(pick, spN - 1) + 1;
      else
        writeStartPosTurns(v, sp, nm);
      s.numTurns = nm;
      s.startTurn = nm;
      s.gameMode = 4;  // FinishedGameData::MODE_SGFPOS
      areaProp = v.d.spInitAreaProp;
      if(v.lane == 0)
        atomicAdd((unsigned long long*)v.d.spGames, 1ull);
      waveSync();
    }
  }
  if(b.initPolicy && areaProp > 0.0f) {
    float u = rng.uni();
    while(u <= 0.0f)
      u = rng.uni();
    s.initLeft = (int)floorf(-dlog(u) * ((float)v.T.A * areaProp));
  }
  if(s.initLeft > 0) {
    s.phase = PH_INIT;
  } else {
    setMoveLimits(v, s, rng, 0.0f);
    s.phase = PH_ROOTEVAL;
  }
  s.rngCtr = rng.ctr;
  s.rootK = 0;
  s.leafKind = LEAF_NONE;
}

// oracle startForkGame: the slot's next game starts from the fork position `b`
// (the finished game replayed to `prefix` moves plus the chosen move); those moves
// stay in the turn records as unsearched turns, no policy initialisation (play.cpp:
// 380-395), mode FORK in the rows (trainingwrite.cpp:468).
KC_D void startForkGame(const GV& v, GameDev& s, const DBoard& b, int prefix, int move) {
  s.rngSeed = mix64(v.d.seed ^ mix64(((uint64_t)(v.d.slotBase + v.g) << 32) | (uint32_t)s.gameNum));
  s.rngCtr = 0;
  s.startGen = *v.d.modelGen;
  s.root = b;
  clearTables(v, s);
  TurnRec* tr = v.turns();
  for(int t = v.lane; t <= prefix; t += 64) {
    const int8_t cell = t < prefix ? tr[t].cell : (int8_t)(move % v.T.A);
    const int8_t dir = t < prefix ? tr[t].dir : (int8_t)(move / v.T.A);
    TurnRec rec;
    memset(&rec, 0, sizeof(rec));
    rec.gen = (uint8_t)*v.d.modelGen;
    rec.cell = cell;
    rec.dir = dir;
    tr[t] = rec;
  }
  s.numTurns = prefix + 1;
  s.startTurn = prefix + 1;
  s.initLeft = 0;
  s.gameMode = 2;
  s.sideCount = 0;
  s.sideNext = 0;
  s.sideMode = 0;
  DRng rng{s.rngSeed, s.rngCtr};
  s.gameHash0 = rng.next();
  s.gameHash1 = rng.next();
  setMoveLimits(v, s, rng, 0.0f);
  s.rngCtr = rng.ctr;
  s.phase = PH_ROOTEVAL;
  s.rootK = 0;
  s.leafKind = LEAF_NONE;
  waveSync();
}

// oracle maybeFork (Play::maybeForkGame play.cpp:1741-1840) at the end of a game, on
// the finished game's stream: an early fork (position after floor(Exp(1) * A *
// earlyForkGameExpectedMoveProp) moves) or a late one (uniform move index); the
// candidates are numChoices uniform draws, with replacement, from the legal moves in
// cell-major order (chooseRandomLegalMoves playutils.cpp:33-60).  Returns true when a
// fork was set up (PH_FORK: one candidate evaluated per round).  No draws at all when
// both probabilities are 0 (SPEC: benchmark mode's streams stay as they are).
KC_D bool maybeFork(const GV& v, GameDev& s, DRng& rng, uint16_t* legal /* LDS [MAX_P] */) {
  const SP& b = v.d.sp;
  if(b.earlyForkProb <= 0.0f && b.forkProb <= 0.0f)
    return false;
  const DTables& T = v.T;
  const bool early = rng.uni() < b.earlyForkProb;
  const bool late = !early && b.forkProb > 0.0f && rng.uni() < b.forkProb;
  if(!early && !late)
    return false;
  const int n = s.numTurns;
  int moveIdx;
  if(early) {
    float u = rng.uni();
    while(u <= 0.0f)
      u = rng.uni();
    moveIdx = (int)floorf(-dlog(u) * (b.earlyForkMoveProp * (float)T.A));
  } else {
    moveIdx = n <= 0 ? 0 : (int)rng.below((uint32_t)n);
  }
  moveIdx = min(moveIdx, max(n - 1, 0));
  // replayGameUpToMove (play.cpp:1703-1739)
  const TurnRec* tr = v.turns();
  DBoard bd;
  boardInit(T, bd);
  for(int t = 0; t < moveIdx; t++) {
    playMoveWave(T, bd, tr[t].cell, tr[t].dir);
    if(bd.finished)
      return false;
  }
  const int maxC = early ? b.earlyForkMaxChoices : b.forkMaxChoices;
  const int numChoices = b.forkMinChoices + (int)rng.below((uint32_t)(maxC - b.forkMinChoices + 1));
  int numLegal = 0;
  for(int base = 0; base < T.P; base += 64) {
    const int q = base + v.lane;  // cell-major: q = cell * 4 + dir
    const bool ok = q < T.P && isLegal(T, bd, q >> 2, q & 3);
    const uint64_t m = ballot(ok);
    if(ok)
      legal[numLegal + __popcll(m & ((1ULL << v.lane) - 1ULL))] = (uint16_t)((q & 3) * T.A + (q >> 2));
    numLegal += __popcll(m);
  }
  waveSync();
  if(numLegal <= 0)
    return false;
  ForkRec* f = v.d.fork + v.g;
  for(int i = 0; i < numChoices; i++) {
    const int k = (int)rng.below((uint32_t)numLegal);
    if(v.lane == 0)
      f->moves[i] = legal[k];
  }
  if(v.lane == 0) {
    f->board = bd;
    f->numChoices = numChoices;
    f->next = 0;
    f->best = -1;
    f->bestWinrate = 0.0f;
    f->prefix = moveIdx;
  }
  s.phase = PH_FORK;
  s.leafKind = LEAF_NONE;
  waveSync();
  return true;
}

// oracle forkEval: the network's value for the position after candidate f.next; the
// best for the player at the fork (first of equals) wins; after the last candidate the
// slot's next game starts from the fork (or normally when the fork move ends the game).
template <int NI>
KC_D void forkEval(const GV& v, GameDev& s, const float* o, float* scratch) {
  ForkRec* f = v.d.fork + v.g;
  float w, l, st;
  float pv[NI];
  postprocess<NI>(v, s.leaf, s.leafSym, o, scratch, w, l, st, scratch, pv);
  const float wr = 0.5f * (w - l + 1.0f);
  const int pla = f->board.pla;
  const int next = f->next;
  int best = f->best;
  float bestWr = f->bestWinrate;
  if(best < 0 || (pla == 2 && wr > bestWr) || (pla == 1 && wr < bestWr)) {
    best = next;
    bestWr = wr;
  }
  waveSync();
  if(v.lane == 0) {
    f->best = best;
    f->bestWinrate = bestWr;
    f->next = next + 1;
  }
  if(next + 1 < f->numChoices)
    return;
  const int move = f->moves[best];
  DBoard bd = f->board;
  playMoveWave(v.T, bd, move % v.T.A, move / v.T.A);
  if(bd.finished)
    startGame(v, s);  // "if the game is over now, don't actually do anything"
  else
    startForkGame(v, s, bd, f->prefix, move);
}

// oracle forkingMove (chooseRandomForkingMove play.cpp:615-633): 70% a temperature-1
// policy move, 25% temperature 2 (chooseRandomPolicyMove playutils.cpp:62-95: policy
// positions in order, probability > 0, not `ban`, chooseIndexWithTemperature), 5% a
// uniform legal move in cell-major order (chooseRandomLegalMove :10-31).  pol: the
// post-processed policy (illegal < 0); cpos / cval / pr: LDS [MAX_P] scratch.
// Returns the policy position, or -1 when there is none.
KC_D int forkingMove(const GV& v, DRng& rng, const float* pol, const DBoard& b, int ban, int* cpos, float* cval,
                     float* pr) {
  const DTables& T = v.T;
  const float r = rng.uni();
  int n = 0;
  if(r < 0.95f) {
    const float temp = r < 0.70f ? 1.0f : 2.0f;
    for(int base = 0; base < T.P; base += 64) {
      const int p = base + v.lane;
      const float q = p < T.P ? pol[p] : -1.0f;
      const bool ok = q > 0.0f && p != ban;
      const uint64_t m = ballot(ok);
      if(ok) {
        const int i = n + __popcll(m & ((1ULL << v.lane) - 1ULL));
        cpos[i] = p;
        cval[i] = q;
      }
      n += __popcll(m);
    }
    waveSync();
    if(n <= 0)
      return -1;
    const int ci = chooseIndex(v, rng, cval, n, temp, pr);
    waveSync();
    return cpos[ci];
  }
  for(int base = 0; base < T.P; base += 64) {
    const int q = base + v.lane;  // cell-major
    const int p = (q & 3) * T.A + (q >> 2);
    const bool ok = q < T.P && p != ban && isLegal(T, b, q >> 2, q & 3);
    const uint64_t m = ballot(ok);
    if(ok)
      cpos[n + __popcll(m & ((1ULL << v.lane) - 1ULL))] = p;
    n += __popcll(m);
  }
  waveSync();
  if(n <= 0)
    return -1;
  const int k = (int)rng.below((uint32_t)n);
  return cpos[k];
}

// A side position `b` joins the game's queue unless it is finished or the queue is full.
KC_D void pushSide(const GV& v, GameDev& s, const DBoard& b) {
  if(b.finished || s.sideCount >= MAX_SIDE)
    return;
  if(v.lane == 0)
    v.d.side[(size_t)v.g * MAX_SIDE + s.sideCount] = b;
  s.sideCount++;
  waveSync();
}

// oracle startSideSearch: the next queued side position becomes the root of a full
// search from a cleared tree (play.cpp:1586-1590: setPosition + runWholeSearchAndGetMove
// with the bot's own parameters).
KC_D void startSideSearch(const GV& v, GameDev& s) {
  s.root = v.d.side[(size_t)v.g * MAX_SIDE + s.sideNext];
  clearTables(v, s);
  s.visitLimit = v.d.sp.maxVisits;
  s.noNoise = 0;
  s.moveWeight = 1.0f;
  s.sideMode = 1;
  s.phase = PH_ROOTEVAL;
  s.rootK = 0;
  s.leafKind = LEAF_NONE;
  waveSync();
}

// After a game's rows: its side positions are searched, then the fork decision and
// the slot's next game (play.cpp:1576-1662, selfplay gameLoop :2008).
// inCommit: called from kCommit, whose kRows has yet to read the finished game's turn records,
// so a start position's records are left to kStartPosTurns (startGame's deferTurns); sideEval
// runs in a round kernel with no kRows pending and lets startGame write them.
KC_D void afterGame(const GV& v, GameDev& s, DRng& rng, uint16_t* scratch, bool inCommit) {
  if(s.sideNext < s.sideCount) {
    startSideSearch(v, s);
    s.rngCtr = rng.ctr;
    return;
  }
  s.sideMode = 0;
  if(!maybeFork(v, s, rng, scratch))
    startGame(v, s, inCommit);
  else
    s.rngCtr = rng.ctr;
}

// oracle emitSideRow (writeGame side rows trainingwrite.cpp:894-937 + addRow with
// isSidePosition, :316-565): the side position's search targets; one value target
// (the search's root value), no next-move policy, no ownership / future boards /
// final run lengths (the reference passes NULL for them; its finalMaxLength
// dereference is B15, here zeros).  History masks from the game stream.
KC_D void emitSideRow(const GV& v, const GameDev& s, const TurnRec& rec, DRng& rng, const DBoard& b, int gameNumMeta) {
  const SearchDev& d = v.d;
  const DTables& T = v.T;
  const int A = T.A, P = T.P, pb = (A + 7) / 8;
  bool h = true;
  uint32_t hm = 0;
  for(int i = 0; i < 5; i++) {
    h = h && rng.uni() < 0.98f;
    hm |= (h ? 1u : 0u) << i;
  }
  unsigned long long r = 0;
  if(v.lane == 0) {
    r = atomicAdd(d.rCount, 1ull);
    if(r >= (unsigned long long)d.rowCap) {
      atomicAdd(d.rCount, (unsigned long long)-1ll);
      atomicAdd(d.rDropped, 1ull);
      r = ~0ull;
    }
  }
  const uint32_t lo = (uint32_t)bcastLane((int)(uint32_t)r, 0), hi = (uint32_t)bcastLane((int)(uint32_t)(r >> 32), 0);
  r = ((unsigned long long)hi << 32) | lo;
  if(r == ~0ull)
    return;
  const int pla = b.pla;
  packRowBinWave(T, b, d.rBin + r * NUM_SPATIAL * pb);
  if(v.lane == 0)
    d.rGlob[r] = (float)T.W;
  const int16_t* sp0 = d.sidePol + (size_t)v.g * P;
  int16_t* pol = d.rPol + r * 2 * P;
  for(int p = v.lane; p < P; p += 64) {
    pol[p] = sp0[p];
    pol[P + p] = (int16_t)1;
  }
  const int li = v.lane;
  float gval = 0.0f;
  if(li < 10)
    gval = (li & 1) ? (pla == 2 ? rec.whiteLoss : rec.whiteWin) : (pla == 2 ? rec.whiteWin : rec.whiteLoss);
  else if(li == 25 || li == 26 || li == 63)
    gval = 1.0f;
  else if(li == 30)
    gval = rec.policySurprise;
  else if(li == 31)
    gval = rec.policyEntropy;
  else if(li == 32)
    gval = rec.searchEntropy;
  else if(li >= 36 && li <= 40)
    gval = ((hm >> (li - 36)) & 1u) ? 1.0f : 0.0f;
  else if(li == 41)
    gval = (float)(s.gameHash0 & 0x3FFFFF);
  else if(li == 42)
    gval = (float)((s.gameHash0 >> 22) & 0x3FFFFF);
  else if(li == 43)
    gval = (float)((s.gameHash0 >> 44) & 0xFFFFF);
  else if(li == 44)
    gval = (float)(s.gameHash1 & 0x3FFFFF);
  else if(li == 45)
    gval = (float)((s.gameHash1 >> 22) & 0x3FFFFF);
  else if(li == 46)
    gval = (float)((s.gameHash1 >> 44) & 0xFFFFF);
  else if(li == 51)
    gval = (float)b.turn;
  else if(li == 53)
    gval = (float)s.startTurn;
  else if(li == 49)
    gval = *d.modelGen != s.startGen ? 1.0f : 0.0f;  // [50]: 0 (searched with the current network)
  else if(li == 55)
    gval = (float)s.gameMode;
  else if(li == 57)
    gval = pla == 2 ? rec.rawWhiteWL : -rec.rawWhiteWL;
  else if(li == 59)
    gval = rec.rawPolicyEntropy;
  else if(li == 60)
    gval = (float)rec.visits;
  d.rGt[r * 64 + li] = gval;
  int8_t* vt = d.rVal + r * 5 * A;
  for(int i = v.lane; i < 5 * A; i += 64)
    vt[i] = 0;
  if(v.lane < 4) {
    const int m = v.lane == 0 ? d.slotBase + v.g : (v.lane == 1 ? gameNumMeta : (v.lane == 2 ? b.turn : s.numTurns));
    d.rMeta[r * 4 + v.lane] = m;
  }
}

// oracle searchTargets: extractPolicyTarget (play.cpp:635-672; scaleMaxToAtLeast 10, no
// direct policy moves) into pt (global [P]) and getPolicySurpriseAndEntropy
// (searchresults.cpp:486-550) at node ni with policy pol.
template <int NI, bool EXPL = false>
KC_D void searchTargets(const GV& v, const SP& sp, const GameDev& s, int ni, const float* pol, bool isRoot,
                        int16_t* pt, TurnRec& rec, int* posv, float* vals, float* tmp, float* tmp2) {
  const int P = v.d.P;
  for(int p = v.lane; p < P; p += 64)
    pt[p] = 0;
  {
    int m = playSelectionValuesAt<NI, EXPL>(v, sp, s, ni, pol, isRoot, 10.0f, false, posv, vals, sp.useLcb);
    float mx = 0.0f;
    for(int i = v.lane; i < m; i += 64)
      mx = vals[i] > mx ? vals[i] : mx;
    mx = waveMax(mx);
    float factor = mx > 30000.0f ? 30000.0f / mx : 1.0f;
    waveSync();
    for(int i = v.lane; i < m; i += 64)
      pt[posv[i]] = (int16_t)roundf(vals[i] * factor);
  }
  waveSync();
  int m = playSelectionValuesAt<NI, EXPL>(v, sp, s, ni, pol, isRoot, 1.0f, true, posv, vals, sp.useLcb);
  const float sumV = seqSum(vals, m, v.lane);
  // per-child terms (0 where the oracle skips), summed in order on lane 0
  waveSync();
  for(int i = v.lane; i < m; i += 64) {
    float p = fmaxf(pol[posv[i]], 1e-30f);
    float tt = vals[i] / sumV;
    float st = 0.0f, et = 0.0f;
    if(tt > 1e-30f) {
      float lt = dlog(tt), lp = dlog(p);
      st = tt * (lt - lp);
      et = -tt * lt;
    }
    tmp[i] = st;
    tmp2[i] = et;
  }
  const float surprise = seqSum(tmp, m, v.lane);
  const float searchEnt = seqSum(tmp2, m, v.lane);
  waveSync();
  for(int p = v.lane; p < P; p += 64) {
    float q = pol[p];
    tmp[p] = q > 1e-30f ? -q * dlog(q) : 0.0f;
  }
  float polEnt = seqSum(tmp, P, v.lane);
  rec.policySurprise = fmaxf(0.0f, surprise);
  rec.searchEntropy = fmaxf(0.0f, searchEnt);
  rec.policyEntropy = fmaxf(0.0f, polEnt);
  waveSync();
}

// oracle valueTargets (extractValueTargets play.cpp:674-682, reportedsearchvalues.cpp:10-50)
KC_D void valueTargets(const Node& n, TurnRec& rec) {
  float wl = fmaxf(-1.0f, fminf(1.0f, n.winLossAvg));
  rec.whiteWin = fmaxf(0.0f, fminf(1.0f, 0.5f * (wl + 1.0f)));
  rec.whiteLoss = fmaxf(0.0f, fminf(1.0f, 0.5f * (-wl + 1.0f)));
  rec.rootWL = wl;
}

// oracle rawStats (computeNNRawStats play.cpp:684-704) from a stored evaluation
KC_D void rawStats(const GV& v, float win, float loss, const float* pol, TurnRec& rec, float* tmp) {
  rec.rawWhiteWL = win - loss;
  for(int p = v.lane; p < v.d.P; p += 64) {
    float q = pol[p];
    tmp[p] = q >= 1e-30f ? -q * dlog(q) : 0.0f;
  }
  // in-order sum of only the q >= 1e-30 terms: zero terms are exact no-ops
  rec.rawPolicyEntropy = seqSum(tmp, v.d.P, v.lane);
  waveSync();
}

// oracle recordTreeRec (recordTreePositionsRec play.cpp:710-814, maxDepth 5), as a
// pre-order walk with an explicit stack: a side row at every non-root node reached
// only through the best moves of the player to move there; excl0/excl1 skipped at the
// root.  Frames and boards live in LDS; every lane walks the same path.
template <int NI, bool EXPL = false>
KC_D void recordTreePositions(const GV& v, const SP& sp, const GameDev& s, DRng& rng, int excl0, int excl1,
                              uint32_t rootVisits, int gameNumMeta, int* posv, float* vals, float* tmp, float* tmp2) {
  constexpr int MAXD = 5;
  __shared__ DBoard tb[MAXD + 1];
  __shared__ int fNode[MAXD + 1], fNext[MAXD + 1], fBest[MAXD + 1], fFlags[MAXD + 1];
  const SearchDev& d = v.d;
  const int A = d.A;
  int16_t* pt = d.sidePol + (size_t)v.g * d.P;
  tb[0] = s.root;
  fNode[0] = s.rootIdx;
  fFlags[0] = 3;  // bit 0: the player to move has played best so far; bit 1: the opponent
  waveSync();
  int depth = 0;
  bool enter = true;
  while(depth >= 0) {
    const int ni = fNode[depth];
    const int k = v.nodes()[ni].numChildren;
    const NodeEdges E = v.edges(ni);
    if(enter) {
      enter = false;
      if(k <= 0) {
        depth--;
        continue;
      }
      if((fFlags[depth] & 1) && ni != s.rootIdx) {
        TurnRec rec;
        searchTargets<NI, EXPL>(v, sp, s, ni, v.pol(ni), false, pt, rec, posv, vals, tmp, tmp2);
        const Node& n = v.nodes()[ni];
        rawStats(v, n.nnWin, n.nnLoss, v.pol(ni), rec, tmp);
        valueTargets(n, rec);
        rec.visits = rootVisits;
        // resolveWeight (play.cpp:1683-1696) when the position is recorded
        const float w = sp.recordTreeWeight;
        const float fl = floorf(w);
        const int copies = (int)fl + (rng.uni() < w - fl ? 1 : 0);
        for(int c = 0; c < copies; c++)
          emitSideRow(v, s, rec, rng, tb[depth], gameNumMeta);
        waveSync();
      }
      if(depth >= MAXD) {
        depth--;
        continue;
      }
      // the most-visited child; children[0]'s count is not consulted (:757-769)
      float bv = -1.0f;
      int bi = BIG;
      for(int i = 1 + v.lane; i < k; i += 64) {
        const float cv = (float)v.nodes()[E[i].child].visits;
        if(cv > bv) {
          bv = cv;
          bi = i;
        }
      }
      waveArgmax(bv, bi);
      fBest[depth] = bv > 0.0f ? bi : 0;
      fNext[depth] = 0;
      waveSync();
    }
    const int flags = fFlags[depth], best = fBest[depth];
    const bool plaB = (flags & 1) != 0, oppB = (flags & 2) != 0;
    int found = -1, foundFlags = 0;
    for(int i = fNext[depth]; i < k; i++) {
      const bool np = oppB, no = plaB && i == best;
      if(!np && !no)
        continue;
      const Edge e = E[i];
      const int mv = (int)e.move;
      if(depth == 0 && (mv == excl0 || mv == excl1))
        continue;
      if((long long)v.nodes()[e.child].visits < (long long)sp.recordTreeThreshold)
        continue;
      found = i;
      foundFlags = (np ? 1 : 0) | (no ? 2 : 0);
      break;
    }
    if(found < 0) {
      depth--;
      continue;
    }
    const Edge e = E[found];
    waveSync();
    fNext[depth] = found + 1;
    tb[depth + 1] = tb[depth];
    waveSync();
    playMoveWave(v.T, tb[depth + 1], (int)e.move % A, (int)e.move / A);
    fNode[depth + 1] = (int)e.child;
    fFlags[depth + 1] = foundFlags;
    waveSync();
    depth++;
    enter = true;
  }
  waveSync();
}

// oracle sideEval: the network's policy at a side position's continuation picks a
// forking move (no ban); the result joins the queue; then the next side position.
template <int NI>
KC_D void sideEval(const GV& v, GameDev& s, const float* o, float* scratch /* LDS [3*MAX_P] */) {
  float w, l, st;
  float pv[NI];
  postprocess<NI>(v, s.leaf, s.leafSym, o, scratch, w, l, st, scratch, pv);
  waveSync();
  DRng rng{s.rngSeed, s.rngCtr};
  // candidates compact in place over the policy (candidate i <= its position)
  const int fm = forkingMove(v, rng, scratch, s.leaf, -1, reinterpret_cast<int*>(scratch + MAX_P), scratch,
                             scratch + 2 * MAX_P);
  if(fm >= 0) {
    DBoard b3 = s.leaf;
    playMoveWave(v.T, b3, fm % v.T.A, fm / v.T.A);
    pushSide(v, s, b3);
  }
  s.sideNext++;
  afterGame(v, s, rng, reinterpret_cast<uint16_t*>(scratch + MAX_P), false);
  waveSync();
}

// oracle finishGame (play.cpp:1431-1460 + trainingwrite.cpp:316-565, 774-890), commit
// part: the SGF move record, the row reservation and the FinRec kRows reads.  The
// turn records and per-turn policies stay in place until the game's next commit,
// so kRows (launched right after this kernel) reads them there.
// oracle resolveTurnWeights: value surprise (play.cpp:1470-1497), surprise-weighted
// target weights (:1498-1574), probabilistic resolution (:1683-1697).  Every lane runs
// the sequential loops on the same data; lane 0 stores each turn's row count.
// Returns the game's number of rows.
KC_D int resolveTurnWeights(const GV& v, const GameDev& s, DRng& rng, float* vs /* LDS [MAX_AREA] */) {
  const SP& b = v.d.sp;
  const int n = s.numTurns, t0 = s.startTurn, A = v.T.A;  // searched turns [t0, n)
  TurnRec* tr = v.turns();
  const float finalWin = s.root.winner == 2 ? 1.0f : (s.root.winner == 1 ? 0.0f : 0.5f);
  float psdw = b.policySurpriseWeight, vsdw = b.valueSurpriseWeight;
  bool reweight = false;
  float sumW = 0.0f, sumPPV = 0.0f, sumVPV = 0.0f, thr = 0.0f;
  if(psdw > 0.0f || vsdw > 0.0f) {
    if(v.lane == 0) {
      const float nowFactor = 1.0f / (1.0f + (float)A * 0.016f);
      float winV = finalWin, lossV = 1.0f - finalWin;
      for(int i = n - 1; i >= t0; i--) {
        winV = winV + nowFactor * (tr[i].whiteWin - winV);
        lossV = lossV + nowFactor * (tr[i].whiteLoss - lossV);
        float x = 0.0f;
        if(winV > 1e-30f)
          x = x + winV * (dlog(winV) - dlog(fmaxf(tr[i].rootNNWin, 1e-30f)));
        if(lossV > 1e-30f)
          x = x + lossV * (dlog(lossV) - dlog(fmaxf(tr[i].rootNNLoss, 1e-30f)));
        if(x < 0.0f)
          x = 0.0f;
        vs[i] = fminf(x, 1.0f);
      }
    }
    waveSync();
    float sumPS = 0.0f, sumVS = 0.0f;
    for(int i = t0; i < n; i++) {
      const float tw = tr[i].targetWeight;
      sumW = sumW + tw;
      sumPS = sumPS + tr[i].policySurprise * tw;
      sumVS = sumVS + vs[i] * tw;
    }
    if(sumW >= 1.0f) {
      reweight = true;
      const float avgPS = sumPS / sumW, avgVS = sumVS / sumW;
      if(avgVS < 0.010f)
        vsdw = vsdw * (avgVS / 0.010f);
      thr = avgPS * 1.5f;
      for(int i = t0; i < n; i++) {
        const float tw = tr[i].targetWeight, ps = tr[i].policySurprise;
        sumPPV = sumPPV + (tw * ps + (1.0f - tw) * fmaxf(0.0f, ps - thr));
        sumVPV = sumVPV + tw * vs[i];
      }
      sumPPV = fmaxf(sumPPV, 1e-10f);
      sumVPV = fmaxf(sumVPV, 1e-10f);
    }
  }
  int total = 0;
  for(int i = t0; i < n; i++) {
    float w = tr[i].targetWeight;
    if(reweight) {
      const float ps = tr[i].policySurprise;
      const float ppv = w * ps + (1.0f - w) * fmaxf(0.0f, ps - thr);
      const float vpv = w * vs[i];
      w = (1.0f - psdw - vsdw) * w + psdw * ppv * sumW / sumPPV + vsdw * vpv * sumW / sumVPV;
    }
    if(w <= 0.0f)
      w = 0.0f;
    const float fl = floorf(w), excess = w - fl;
    const int rows = (int)(rng.uni() < excess ? fl + 1.0f : fl);
    total += rows;
    waveSync();
    if(v.lane == 0)
      tr[i].rows = (uint8_t)rows;
  }
  waveSync();
  return total;
}

// MATCH: the record also carries the candidate's colour, and no rows are reserved (match
// play writes none: kRows does not run and nothing counts as dropped).  The turn weights
// are still resolved, so the game stream advances as in self-play.
template <bool MATCH>
KC_D void finishGameRecord(const GV& v, const GameDev& s, DRng& rng, float* scratch) {
  const SearchDev& d = v.d;
  const int numMoves = s.numTurns;
  const TurnRec* tr = v.turns();
  const int numRows = resolveTurnWeights(v, s, rng, scratch);
  {
    // the game's move record (SGF)
    unsigned long long gi = 0;
    if(v.lane == 0) {
      gi = atomicAdd(d.gCount, 1ull);
      if(gi >= (unsigned long long)d.gCap) {
        atomicAdd(d.gCount, (unsigned long long)-1ll);
        atomicAdd(d.gDropped, 1ull);
      }
    }
    gi = (unsigned long long)(uint32_t)bcastLane((int)(uint32_t)gi, 0);
    if(gi < (unsigned long long)d.gCap) {
      GameRec* gr = d.gRec + gi;
      if(v.lane == 0) {
        gr->slot = d.slotBase + v.g;
        gr->gameNum = (int32_t)s.gameNum;
        gr->numMoves = numMoves;
        gr->winner = s.root.winner;
        gr->candidate = MATCH ? matchCandidateColour(d.slotBase + v.g, (int)s.gameNum) : 0;
      }
      for(int t = v.lane; t < numMoves; t += 64) {
        gr->cell[t] = (uint8_t)tr[t].cell;
        gr->dir[t] = (uint8_t)tr[t].dir;
      }
    }
  }
  if constexpr(MATCH)
    return;
  if(v.lane == 0) {
    unsigned long long base = atomicAdd(d.rCount, (unsigned long long)numRows);
    bool fits = true;
    if(base + (unsigned long long)numRows > (unsigned long long)d.rowCap) {
      atomicAdd(d.rCount, (unsigned long long)(-(long long)numRows));
      atomicAdd(d.rDropped, (unsigned long long)numRows);
      fits = false;
    }
    FinRec* f = d.fin + v.g;
    f->rngSeed = rng.seed;
    f->rngCtr = rng.ctr;
    f->gameHash0 = s.gameHash0;
    f->gameHash1 = s.gameHash1;
    f->rowBase = base;
    f->numMoves = numMoves;
    f->numRows = numRows;
    f->startTurn = s.startTurn;
    f->gameMode = s.gameMode;
    f->genStart = s.startGen;
    f->genEnd = *d.modelGen;
    f->winner = s.root.winner;
    f->gameNum = s.gameNum;
    f->pending = fits && numRows > 0 ? 1 : 0;
  }
}

// kRows: the training rows of the games the preceding kCommit finished
// (trainingwrite.cpp:316-565 addRow via writeGame :774-890; turn t is written
// TurnRec::rows times).  One 256-thread block per committed game; the boards after
// every move, the row -> turn map and the final board's per-cell max runs are built
// once in LDS, then wave w writes rows w, w + 4, ...
constexpr int ROWS_WAVES = 8;
__global__ void __launch_bounds__(64 * ROWS_WAVES) kRows(const SearchDev* __restrict__ dp,
                                                         const DTables* __restrict__ Tp) {
  const SearchDev& d = *dp;
  if((int)blockIdx.x >= *d.commitCount)
    return;
  const int g = d.commitList[blockIdx.x];
  FinRec* fp = d.fin + g;
  if(fp->pending != 1)
    return;
  const FinRec f = *fp;
  const DTables& T = *Tp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  GV v(d, T, g);
  __shared__ DBoard boards[MAX_AREA + 1];
  __shared__ float tWin[MAX_AREA + 1], tLoss[MAX_AREA + 1];
  __shared__ int8_t finRun[MAX_AREA];
  __shared__ uint8_t hMask[2 * MAX_AREA];
  __shared__ uint8_t rowTurn[2 * MAX_AREA];
  __shared__ uint8_t tCell[MAX_AREA], tDir[MAX_AREA], tRows[MAX_AREA];
  const int numMoves = f.numMoves, numRows = min(f.numRows, 2 * MAX_AREA);  // <= 2 numMoves by construction
  const int A = T.A, P = T.P, pb = (A + 7) / 8;
  const TurnRec* tr = v.turns();
  const float finalWin = f.winner == 2 ? 1.0f : (f.winner == 1 ? 0.0f : 0.5f);
  // the turn records into LDS in parallel; the serial steps below then read LDS only
  for(int t = threadIdx.x; t < numMoves; t += 64 * ROWS_WAVES) {
    const TurnRec rec = tr[t];
    tWin[t] = rec.whiteWin;
    tLoss[t] = rec.whiteLoss;
    tCell[t] = (uint8_t)rec.cell;
    tDir[t] = (uint8_t)rec.dir;
    tRows[t] = rec.rows;
  }
  __syncthreads();
  if(threadIdx.x == 0) {
    tWin[numMoves] = finalWin;
    tLoss[numMoves] = 1.0f - finalWin;
    DBoard b;
    boardInit(T, b);
    boards[0] = b;
    for(int t = 0; t < numMoves; t++) {
      applyMove(T, b, tCell[t], tDir[t]);
      boards[t + 1] = b;
    }
    int j = 0;
    for(int t = 0; t < numMoves; t++)
      for(int c = 0; c < (int)tRows[t] && j < 2 * MAX_AREA; c++)
        rowTurn[j++] = (uint8_t)t;
    // history-mask draws, in row order from the game's stream (the chain stops
    // drawing at its first failure, so the draws are consumed sequentially)
    DRng rng{f.rngSeed, f.rngCtr};
    for(int r = 0; r < numRows; r++) {
      bool h = true;
      uint32_t hm = 0;
      for(int i = 0; i < 5; i++) {
        h = h && rng.uni() < 0.98f;
        hm |= (h ? 1u : 0u) << i;
      }
      hMask[r] = (uint8_t)hm;
    }
  }
  __syncthreads();
  const DBoard& fin = boards[numMoves];
  for(int c = threadIdx.x; c < A; c += 64 * ROWS_WAVES)
    finRun[c] = colorAt(fin, c) == 0 ? 0 : (int8_t)maxRun(T, fin, c);
  __syncthreads();
  const float nowF1 = 1.0f / (1.0f + (float)A * 0.176f), nowF2 = 1.0f / (1.0f + (float)A * 0.056f),
              nowF3 = 1.0f / (1.0f + (float)A * 0.016f);
  for(int row = wave; row < numRows; row += ROWS_WAVES) {
    const int t = rowTurn[row];
    const uint32_t hm = hMask[row];
    const size_t r = (size_t)f.rowBase + row;
    const DBoard& b = boards[t];
    const int pla = b.pla, opp = 3 - pla;
    packRowBinWave(T, b, d.rBin + r * NUM_SPATIAL * pb);
    if(lane == 0)
      d.rGlob[r] = (float)T.W;
    const int16_t* p0 = v.turnPol(t);
    const int16_t* p1 = t + 1 < numMoves ? v.turnPol(t + 1) : nullptr;
    int16_t* pol = d.rPol + r * 2 * P;
    for(int p = lane; p < P; p += 64) {
      pol[p] = p0[p];
      pol[P + p] = p1 ? p1[p] : (int16_t)1;
    }
    float gval = 0.0f;
    const int li = lane;
    if(li < 10) {
      const int fi = li >> 1;
      const float nf = fi == 0 ? 0.0f : (fi == 1 ? nowF1 : (fi == 2 ? nowF2 : (fi == 3 ? nowF3 : 1.0f)));
      float win = 0.0f, loss = 0.0f, left = 1.0f;
      for(int i = t; i <= numMoves; i++) {
        float now;
        if(i == numMoves) {
          now = left;
          left = 0.0f;
        } else {
          now = left * nf;
          left = left * (1.0f - nf);
        }
        win = win + now * (pla == 2 ? tWin[i] : tLoss[i]);
        loss = loss + now * (pla == 2 ? tLoss[i] : tWin[i]);
      }
      gval = (li & 1) ? loss : win;
    } else if(li == 22) {
      float sum = 0.0f;
      for(int i = t + 1; i <= numMoves; i++) {
        float prevWL = tWin[i - 1] - tLoss[i - 1], nextWL = tWin[i] - tLoss[i];
        float var = (nextWL - prevWL) * (nextWL - prevWL);
        sum = sum + (float)(i - t) * var;
      }
      gval = sum;
    } else if(li == 25 || li == 26 || li == 27 || li == 33 || li == 63) {
      gval = 1.0f;
    } else if(li == 28) {
      gval = t + 1 < numMoves ? 1.0f : 0.0f;
    } else if(li == 30) {
      gval = tr[t].policySurprise;
    } else if(li == 31) {
      gval = tr[t].policyEntropy;
    } else if(li == 32) {
      gval = tr[t].searchEntropy;
    } else if(li >= 36 && li <= 40) {
      gval = ((hm >> (li - 36)) & 1u) ? 1.0f : 0.0f;
    } else if(li == 41) {
      gval = (float)(f.gameHash0 & 0x3FFFFF);
    } else if(li == 42) {
      gval = (float)((f.gameHash0 >> 22) & 0x3FFFFF);
    } else if(li == 43) {
      gval = (float)((f.gameHash0 >> 44) & 0xFFFFF);
    } else if(li == 44) {
      gval = (float)(f.gameHash1 & 0x3FFFFF);
    } else if(li == 45) {
      gval = (float)((f.gameHash1 >> 22) & 0x3FFFFF);
    } else if(li == 46) {
      gval = (float)((f.gameHash1 >> 44) & 0xFFFFF);
    } else if(li == 51) {
      gval = (float)t;
    } else if(li == 53) {
      gval = (float)f.startTurn;
    } else if(li == 49) {
      // earlier-network metadata (trainingwrite.cpp:459-461, :844-850): the game saw a
      // hot reload; reloads after this turn's commit
      gval = f.genEnd != f.genStart ? 1.0f : 0.0f;
    } else if(li == 50) {
      gval = (float)(uint8_t)((uint32_t)f.genEnd - (uint32_t)tr[t].gen);
    } else if(li == 55) {
      gval = (float)f.gameMode;
    } else if(li == 57) {
      gval = pla == 2 ? tr[t].rawWhiteWL : -tr[t].rawWhiteWL;
    } else if(li == 59) {
      gval = tr[t].rawPolicyEntropy;
    } else if(li == 60) {
      gval = (float)tr[t].visits;
    }
    d.rGt[r * 64 + li] = gval;
    int8_t* vt = d.rVal + r * 5 * A;
    const DBoard& b2 = boards[min(t + 2, numMoves)];
    const DBoard& b3 = boards[min(t + 6, numMoves)];
    for(int c = lane; c < A; c += 64) {
      int fc = colorAt(fin, c), c2 = colorAt(b2, c), c3 = colorAt(b3, c);
      vt[c] = fc == pla ? 1 : (fc == opp ? -1 : 0);
      vt[A + c] = 0;
      vt[2 * A + c] = c2 == pla ? 1 : (c2 == opp ? -1 : 0);
      vt[3 * A + c] = c3 == pla ? 1 : (c3 == opp ? -1 : 0);
      vt[4 * A + c] = finRun[c];
    }
    if(lane < 4) {
      int m = lane == 0 ? d.slotBase + g : (lane == 1 ? f.gameNum : (lane == 2 ? t : numMoves));
      d.rMeta[r * 4 + lane] = m;
    }
  }
  __syncthreads();
  if(threadIdx.x == 0)
    fp->pending = 0;
}

// oracle commitMove (getChosenMoveLoc searchresults.cpp:435-453, extract*Targets
// play.cpp:635-704, getPolicySurpriseAndEntropy searchresults.cpp:486-550, makeMove)
// MATCH (two-network match play): the game record carries the candidate's colour and no
// rows are emitted; the config admits no side positions, forks or tree positions there.
template <int NI, bool MATCH = false, bool EXPL = false>
__global__ void __launch_bounds__(64) kCommit(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  const SearchDev& d = *dp;
  if((int)blockIdx.x >= *d.commitCount)
    return;
  const int g = d.commitList[blockIdx.x];
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int* posv = reinterpret_cast<int*>(lds);                    // [MAX_P]
  float* vals = reinterpret_cast<float*>(posv + MAX_P);       // [MAX_P]
  float* tmp = vals + MAX_P;                                  // [MAX_P]
  float* tmp2 = tmp + MAX_P;                                  // [MAX_P]
  int* qtail = reinterpret_cast<int*>(tmp2 + MAX_P);
  uint32_t* liveBits = reinterpret_cast<uint32_t*>(qtail + 4);  // [cap/32]
  uint16_t* queue = reinterpret_cast<uint16_t*>(liveBits + d.cap / 32);     // [cap]
  __shared__ GameDev s;
  GV v(d, *Tp, g);
  SPROF_INIT();
  [[maybe_unused]] const unsigned long long t0 = SPROF_NOW();
  loadGame<MATCH>(v, s);
  // MATCH: the mover's own parameters (per-side settings; equal to d.sp without them)
  const SP& sp = MATCH ? *v.sp : d.sp;
  const int P = d.P, A = d.A;
  DRng rng{s.rngSeed, s.rngCtr};
  if(s.root.finished) {
    // a policy-initialisation move ended the game: nothing was searched, no rows
    // (the reference's main loop does not run, play.cpp:1262-1264)
    finishGameRecord<MATCH>(v, s, rng, reinterpret_cast<float*>(lds) + 2 * MAX_P);
    s.gamesFinished++;
    s.gameNum++;
    s.sideNext = 0;
    afterGame(v, s, rng, reinterpret_cast<uint16_t*>(lds), true);
    matchMoveLimits<MATCH>(v, s);
    waveSync();
    storeGame(v, s);
    return;
  }
  // a side position's search (play.cpp:1576-1662) ends like a move search, but
  // writes one row and plays nothing
  const bool side = s.sideMode != 0;
  // move choice: self-play disables LCB for the game's moves (runBotWithLimits
  // play.cpp:1040-1046), not for a side position's response (:1590)
  int n = playSelectionValues<NI, EXPL>(v, *v.sp, s, 0.0f, true, posv, vals, side ? sp.useLcb != 0 : false);
  if(n <= 0) {
    s.err = ERR_NO_CANDIDATE;
    n = 1;
    posv[0] = 0;
  }
  const float temp = interpolateEarly(v.T, s.root.turn, sp.moveTempHalflife, sp.moveTempEarly, sp.moveTemp);
  int ci = chooseIndex(v, rng, vals, n, temp, tmp);
  waveSync();
  const int chosen = posv[ci];
  const Node& r = v.nodes()[s.rootIdx];
  TurnRec rec;
  valueTargets(r, rec);
  rec.visits = r.visits;
  rec.rootNNWin = r.nnWin;
  rec.rootNNLoss = r.nnLoss;
  rec.targetWeight = s.moveWeight;
  rec.rows = 0;
  rec.gen = (uint8_t)*v.d.modelGen;
  const int t = s.numTurns;
  int16_t* pt = side ? d.sidePol + (size_t)g * P : v.turnPol(t);
  waveSync();
  // the targets run after runBotWithLimits restored the base parameters (play.cpp:1066, :1307-1320)
  searchTargets<NI, EXPL>(v, sp, s, s.rootIdx, v.rootNoised(), true, pt, rec, posv, vals, tmp, tmp2);
  rawStats(v, s.rawWin, s.rawLoss, v.rawPolicy(), rec, tmp);
  const bool recordTree = sp.recordTree != 0 && sp.recordTreeWeight > 0.0f;
  if(side) {
    emitSideRow(v, s, rec, rng, s.root, s.gameNum - 1);
    // its subtree positions (play.cpp:1612-1628)
    if(recordTree)
      recordTreePositions<NI, EXPL>(v, sp, s, rng, -1, -1, r.visits, s.gameNum - 1, posv, vals, tmp, tmp2);
    // occasionally continue: the response, then a forking move from the network's
    // policy there becomes another side position (play.cpp:1632-1656)
    if(rng.uni() < 0.25f) {
      DBoard b2 = s.root;
      playMoveWave(v.T, b2, chosen % A, chosen / A);
      if(!b2.finished) {
        s.leaf = b2;
        s.phase = PH_SIDEEVAL;
        s.rngCtr = rng.ctr;
        waveSync();
        storeGame(v, s);
        return;
      }
    }
    s.sideNext++;
    afterGame(v, s, rng, reinterpret_cast<uint16_t*>(posv), true);
    waveSync();
    storeGame(v, s);
    return;
  }
  // a side position: the root policy's alternative to the move (play.cpp:1328-1345)
  int forkMove = -1;
  if(sp.sideProb > 0.0f && rng.uni() < sp.sideProb) {
    const int fm = forkingMove(v, rng, v.pol(s.rootIdx), s.root, chosen, posv, vals, tmp);
    forkMove = fm;
    if(fm >= 0) {
      DBoard b2 = s.root;
      playMoveWave(v.T, b2, fm % A, fm / A);
      pushSide(v, s, b2);
    }
  }
  // subtree positions of this search, except the played and the forked branches
  // (play.cpp:1347-1361)
  if(recordTree) {
    waveSync();
    recordTreePositions<NI, EXPL>(v, sp, s, rng, chosen, forkMove, r.visits, s.gameNum, posv, vals, tmp, tmp2);
  }
  rec.cell = (int8_t)(chosen % A);
  rec.dir = (int8_t)(chosen / A);
  for(int i = 0; i < 5; i++)
    rec.pad[i] = 0;
  waveSync();
  if(v.lane == 0)
    v.turns()[t] = rec;
  s.numTurns++;
  [[maybe_unused]] const unsigned long long t1 = SPROF_NOW();
  SPROF_ADD(18, t1 - t0);
  playMoveWave(v.T, s.root, chosen % A, chosen / A);
  s.moves++;
  waveSync();
  if(s.root.finished) {
    [[maybe_unused]] const unsigned long long t3 = SPROF_NOW();
    finishGameRecord<MATCH>(v, s, rng, tmp);
    [[maybe_unused]] const unsigned long long t4 = SPROF_NOW();
    s.gamesFinished++;
    s.gameNum++;
    s.sideNext = 0;
    waveSync();
    afterGame(v, s, rng, reinterpret_cast<uint16_t*>(posv), true);
    SPROF_ADD(20, t4 - t3);
    SPROF_ADD(21, SPROF_NOW() - t4);
    SPROF_ADD(23, 1);
  } else {
    // the next move's limits decide whether its search starts from a cleared tree
    if(setMoveLimits(v, s, rng, rec.rootWL))
      clearTables(v, s);
    else
      reuseTree(v, s, chosen, liveBits, queue, qtail);
    [[maybe_unused]] const unsigned long long t2 = SPROF_NOW();
    SPROF_ADD(19, t2 - t1);
    SPROF_ADD(22, s.liveCount);
    s.rngCtr = rng.ctr;
    s.phase = PH_ROOTEVAL;
    s.rootK = 0;
  }
  // the next search's limit by its mover: the other side, or after a game's end the next
  // game's first mover (the colours, and with them the sides, have swapped)
  matchMoveLimits<MATCH>(v, s);
  waveSync();
  storeGame(v, s);
  SPROF_ADD(16, 1);
  SPROF_ADD(17, SPROF_NOW() - t0);
  SPROF_FLUSH();
}

// After kCommit (and kRows) with a start-position table set: the committed games whose next
// game kCommit started from a sample get the sample's moves as turn records now that kRows
// has read the finished game's.  One wave per commit-list entry.
__global__ void __launch_bounds__(64) kStartPosTurns(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  const SearchDev& d = *dp;
  if((int)blockIdx.x >= *d.commitCount)
    return;
  const int g = d.commitList[blockIdx.x];
  GameDev* gs = d.games + g;
  const int pend = __builtin_amdgcn_readfirstlane(gs->spPending);
  const int spN = d.spN;
  if(pend <= 0 || spN <= 0)
    return;
  GV v(d, *Tp, g);
  const coffee_start_position* sp = d.spTable + min(pend - 1, spN - 1);
  // the replay played numTurns moves when the game started in this launch's kCommit; nothing
  // has run for the game since
  const int nm = min(max(__builtin_amdgcn_readfirstlane(gs->numTurns), 0), min(d.A - 1, COFFEE_ANALYSIS_MAX_MOVES));
  writeStartPosTurns(v, sp, nm);
  waveSync();
  if(v.lane == 0)
    gs->spPending = 0;
}

// kCompact: the list of games whose row the network evaluates this round, at most
// d.nnCap rows (one full wave of network workgroups: a launch's cost steps with its
// number of workgroup waves).  The needing games are taken in cyclic game order from
// the round-robin pointer *d.nnRR, which moves past the last game taken whenever the
// cap bites, so a deferred row waits at most ceil(G / cap) rounds.  Rows past the cap
// are deferred (nnDefer): their games keep their leaf and skip the next select.  The
// oracle applies the same rule (ora_search.cpp selfplayRound).
// accumulate != 0: the count is also added to *d.nnTimedEvals (sampled kernel timing).
// Layout: the games are cut into 64-game chunks; wave w owns the contiguous chunks
// [w * cpw, (w + 1) * cpw) and lane l game l of each, so every load and every nnDefer
// store is one coalesced 256-byte access per chunk.  The need flags and cache bids of
// all of a lane's chunks are loaded before the first use (up to CP_CH chunks per wave),
// so the kernel waits for one round of loads.  Positions: a lane's packed count (high
// half: needing games at or past the round-robin pointer, low half: the others, G <
// 65536) is summed over the wave and scanned over the waves; inside a wave the chunks
// are walked in order with a ballot per chunk.
// (256 threads cover a group of 8192 games: a 4-wave workgroup finds room beside the
// other group's network kernels, where a 1024-thread one waited for a whole CU to
// drain: 34 us per launch at C3)
constexpr int CP_CH = 32;
// resolve != 0 (after a fused kBackupSelect): the block first does kResolve's work -- the
// round winners' tags cleared by every thread, the pending selections completed by waves
// 0-3 -- and the compaction below reads the need flags and bids those selections wrote
// after a workgroup barrier: one dispatch fewer on every fused round.
constexpr int CP_RESOLVE_WAVES = 4;
// (The resolving instance alone holds the LDS game copies: the plain one, which the separate
// round kernels and the default precision's network run beside, keeps its 132 bytes of LDS
// and fits on a CU next to any network workgroup.)
//
// Match play (MATCH; never after a fused round): the same pass with four running counts,
// net x (at or past the pointer / before it), as four 16-bit fields of a 64-bit word
// (bits 48.. net 1 past, 32.. net 0 past, 16.. net 1 before, 0.. net 0 before) and the
// same ballot walk.  The cap rule is the single-net one on both nets' rows together: a
// row's joint position (both nets' fields added) decides whether it is taken, deferred
// and where the pointer moves; a taken row goes to its own net's list (nnIdx / nnIdx1) at
// its position among that net's rows, so each list keeps the joint order, and bids in its
// net's cache.  The net comes from netOf on the game's stored state, read for needing
// games only.  Same 256-thread launch; the 64-bit partial sums take 272 bytes of LDS
// instead of 144 and no game copy, so the workgroup still fits beside any network one.
template <int NI>
KC_D void compactMatch(const SearchDev& d, int accumulate) {
  __shared__ uint64_t wsum[16], wpre[17];
  const int nt = blockDim.x, nw = nt >> 6;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nch = (d.G + 63) >> 6;
  const int cpw = (nch + nw - 1) / nw;  // <= 64 chunks per wave, as in the single-net pass
  const int g0 = w * cpw * 64 + lane;
  const int p = *d.nnRR;
  // the two nets' lists and cache tags as plain (wave-uniform) pointers: a lane picks by its game's net
  int32_t* const idxOf[2] = {d.nnIdx, d.nnIdx1};
  uint32_t* const tagOf[2] = {cacheOf<true>(d, 0).tag, cacheOf<true>(d, 1).tag};
  uint64_t need = 0, net1 = 0;  // bit k: game g0 + 64 k needs the network / is evaluated by net 1
  for(int k = 0; k < cpw; k++) {
    const int i = g0 + 64 * k;
    if(i < d.G && d.nnNeed[i]) {
      need |= 1ull << k;
      net1 |= (uint64_t)netOf(d, i, d.games[i]) << k;
    }
  }
  const uint64_t atOrPast = p <= g0 ? ~0ull : (p - g0 > 64 * 63 ? 0ull : ~0ull << ((p - g0 + 63) / 64));
  uint64_t c = ((uint64_t)__popcll(need & atOrPast & net1) << 48) + ((uint64_t)__popcll(need & atOrPast & ~net1) << 32) +
               ((uint64_t)__popcll(need & ~atOrPast & net1) << 16) + (uint64_t)__popcll(need & ~atOrPast & ~net1);
#pragma unroll
  for(int off = 32; off >= 1; off >>= 1)
    c += (uint64_t)__shfl_xor((long long)c, off, 64);
  if(lane == 0)
    wsum[w] = c;
  __syncthreads();
  if(t < 64) {
    uint64_t x = t < nw ? wsum[t] : 0ull, xi = x;
#pragma unroll
    for(int off = 1; off < 16; off <<= 1) {
      const uint64_t v = (uint64_t)__shfl_up((long long)xi, off, 64);
      if(t >= off)
        xi += v;
    }
    if(t < 16)
      wpre[t] = xi - x;
    if(t == 15)
      wpre[16] = xi;
  }
  __syncthreads();
  const uint64_t all = wpre[16], excl = wpre[w];
  auto field = [](uint64_t x, int f) { return (int)((x >> (16 * f)) & 0xFFFFull); };
  // per net n: rows at or past the pointer in all, and this wave's running positions
  const int hiAll[2] = {field(all, 2), field(all, 3)};
  const int totalHi = hiAll[0] + hiAll[1];
  const int total = totalHi + field(all, 0) + field(all, 1), cap = d.nnCap;
  int oh[2] = {field(excl, 2), field(excl, 3)};
  int ol[2] = {hiAll[0] + field(excl, 0), hiAll[1] + field(excl, 1)};
  const int taken = min(total, cap);
  const uint64_t below = (1ull << lane) - 1ull;
  for(int k = 0; k < cpw; k++) {
    const int i = g0 + 64 * k;
    const bool nd = (need >> k) & 1u;
    const int n = (int)((net1 >> k) & 1u);
    const bool past = i >= p;
    const uint64_t b1 = ballot(nd && n == 1), b0 = ballot(nd && n == 0);
    const uint64_t g1 = ballot(nd && n == 1 && past), g0b = ballot(nd && n == 0 && past);
    if(nd) {
      // position among the net's own rows and among both nets' rows, in cyclic game order
      const int own = past ? oh[n] + __popcll((n ? g1 : g0b) & below)
                           : ol[n] + __popcll((n ? b1 & ~g1 : b0 & ~g0b) & below);
      const int other = past ? oh[1 - n] + __popcll((n ? g0b : g1) & below)
                             : ol[1 - n] + __popcll((n ? b0 & ~g0b : b1 & ~g1) & below);
      const int pos = own + other;
      const bool in = pos < cap;
      if(in) {
        (n ? idxOf[1] : idxOf[0])[own] = i;  // own <= pos < cap <= G
        const uint32_t bid = d.nnBid[i];
        if(bid != ~0u)
          atomicMax(&(n ? tagOf[1] : tagOf[0])[bid], (uint32_t)i + 1u);
      }
      d.nnDefer[i] = in ? 0 : 1;
      if(total > cap && pos == cap - 1)
        *d.nnRR = i + 1 < d.G ? i + 1 : 0;
      if(pos == taken - 1) {
        // the last row taken: its net's list ends with it, the other list holds the rest
        const int cn[2] = {n ? taken - own - 1 : own + 1, n ? own + 1 : taken - own - 1};
        *d.nnCount = cn[0];
        *d.nnCount1 = cn[1];
        d.nnPeak[0] = max(d.nnPeak[0], cn[0]);
        d.nnPeak[1] = max(d.nnPeak[1], cn[1]);
        d.nnNetEvals[0] += (unsigned long long)cn[0];
        d.nnNetEvals[1] += (unsigned long long)cn[1];
      }
    } else if(i < d.G) {
      d.nnDefer[i] = 0;
    }
    oh[0] += __popcll(g0b);
    oh[1] += __popcll(g1);
    ol[0] += __popcll(b0 & ~g0b);
    ol[1] += __popcll(b1 & ~g1);
  }
  if(t == nt - 1) {
    if(total == 0) {
      *d.nnCount = 0;
      *d.nnCount1 = 0;
    }
    *d.pendCount = 0;
    if(accumulate)
      *d.nnTimedEvals += (unsigned long long)taken;
  }
}

template <int NI, bool RESOLVE, bool MATCH = false>
__global__ void __launch_bounds__(1024) kCompact(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp,
                                                 int accumulate) {
  const SearchDev& d = *dp;
  if constexpr(MATCH) {
    static_assert(!RESOLVE, "match play runs no fused rounds");
    compactMatch<NI>(d, accumulate);
    return;
  }
  __shared__ uint32_t wsum[16], wpre[17];
  const int nt = blockDim.x, nw = nt >> 6;  // 256 or 1024 threads (launchCompact)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if constexpr(RESOLVE) {
    __shared__ GameDev rs[CP_RESOLVE_WAVES];
    clearRoundTags(d, t, nt);
    if(w < CP_RESOLVE_WAVES)
      completePending<NI>(d, *Tp, w, CP_RESOLVE_WAVES, rs[w]);
    __syncthreads();
  }
  const int nch = (d.G + 63) >> 6;
  const int cpw = (nch + nw - 1) / nw;  // chunks per wave (<= 64: G < 65536, >= 16 waves past 8192 games)
  const int g0 = w * cpw * 64 + lane;   // this lane's game in the wave's first chunk
  const int p = *d.nnRR;
  const bool vec = cpw <= CP_CH;
  uint64_t need = 0;  // bit k: game g0 + 64 k needs the network
  uint32_t bids[CP_CH];
  if(vec) {
#pragma unroll
    for(int k = 0; k < CP_CH; k++) {
      bids[k] = ~0u;
      if(k < cpw) {
        const int i = g0 + 64 * k;
        const int ic = i < d.G ? i : 0;
        bids[k] = d.nnBid[ic];
        need |= (uint64_t)(i < d.G && d.nnNeed[ic] ? 1u : 0u) << k;
      }
    }
  } else {
    for(int k = 0; k < cpw; k++) {
      const int i = g0 + 64 * k;
      need |= (uint64_t)(i < d.G && d.nnNeed[i] ? 1u : 0u) << k;
    }
  }
  // bit k of atOrPast: game g0 + 64 k >= p
  const uint64_t atOrPast = p <= g0 ? ~0ull : (p - g0 > 64 * 63 ? 0ull : ~0ull << ((p - g0 + 63) / 64));
  uint32_t c = ((uint32_t)__popcll(need & atOrPast) << 16) + (uint32_t)__popcll(need & ~atOrPast);
#pragma unroll
  for(int off = 32; off >= 1; off >>= 1)
    c += (uint32_t)__shfl_xor((int)c, off, 64);
  if(lane == 0)
    wsum[w] = c;
  __syncthreads();
  if(t < 64) {
    uint32_t x = t < nw ? wsum[t] : 0u, xi = x;
#pragma unroll
    for(int off = 1; off < 16; off <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)xi, off, 64);
      if(t >= off)
        xi += v;
    }
    if(t < 16)
      wpre[t] = xi - x;
    if(t == 15)
      wpre[16] = xi;
  }
  __syncthreads();
  const uint32_t all = wpre[16], excl = wpre[w];
  const int totalHi = (int)(all >> 16), total = totalHi + (int)(all & 0xFFFFu), cap = d.nnCap;
  int oh = (int)(excl >> 16), ol = totalHi + (int)(excl & 0xFFFFu);  // wave-uniform running positions
  const uint64_t below = (1ull << lane) - 1ull;
  auto chunk = [&](int k, uint32_t bid) {
    const int i = g0 + 64 * k;
    const bool nd = (need >> k) & 1u;
    const uint64_t b = ballot(nd), ge = ballot(nd && i >= p);
    if(nd) {
      const int pos = i >= p ? oh + __popcll(ge & below) : ol + __popcll(b & ~ge & below);
      const bool in = pos < cap;
      if(in) {
        d.nnIdx[pos] = i;
        // the evaluation's bid for its NN-cache slot (kBackup: the highest game stores it)
        if(bid != ~0u)
          atomicMax(&d.cTag[bid], (uint32_t)i + 1u);
      }
      d.nnDefer[i] = in ? 0 : 1;
      if(total > cap && pos == cap - 1)
        *d.nnRR = i + 1 < d.G ? i + 1 : 0;
    } else if(i < d.G) {
      d.nnDefer[i] = 0;
    }
    oh += __popcll(ge);
    ol += __popcll(b & ~ge);
  };
  if(vec) {
#pragma unroll
    for(int k = 0; k < CP_CH; k++)
      if(k < cpw)
        chunk(k, bids[k]);
  } else {
    for(int k = 0; k < cpw; k++) {
      const int i = g0 + 64 * k;
      chunk(k, i < d.G ? d.nnBid[i] : ~0u);
    }
  }
  if(t == nt - 1) {
    const int count = min(total, cap);
    *d.nnCount = count;
    *d.pendCount = 0;  // the pending list kResolve (or the resolve phase above) completed
    if(accumulate)
      *d.nnTimedEvals += (unsigned long long)count;
  }
}

__global__ void __launch_bounds__(64) kInit(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  const SearchDev& d = *dp;
  const int g = blockIdx.x;
  if(g >= d.G)
    return;
  __shared__ GameDev s;
  GV v(d, *Tp, g);
  for(int i = v.lane; i < (int)(sizeof(GameDev) / 4); i += 64)
    reinterpret_cast<uint32_t*>(&s)[i] = 0;
  waveSync();
  s.svbSel = 0;
  s.gameNum = 0;
  startGame(v, s);
  // benchmark stagger: idle rounds before the slot's first game, so game ends (and
  // row bursts) spread over the run instead of arriving in phase; own stream, so
  // the games themselves are unchanged
  s.startDelay = d.startStagger > 0
                     ? (int32_t)(mix64(d.seed ^ 0x5a5a5a5a5a5a5a5aULL ^ (uint64_t)(d.slotBase + g)) %
                                 (uint64_t)d.startStagger)
                     : 0;
  waveSync();
  storeGame(v, s);
}

// Per-side match settings, after kInit: a first game whose first mover is side 1 searches
// to side 1's limit (kInit's startGame gave side 0's).  One thread per game.
__global__ void __launch_bounds__(256) kMatchSideLimits(const SearchDev* __restrict__ dp) {
  const SearchDev& d = *dp;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if(g >= d.G)
    return;
  GameDev* s = d.games + g;
  if(matchNet(d.slotBase + g, s->gameNum, s->root.pla))
    s->visitLimit = d.sp1.maxVisits;
}

// Canonical breadth-first export of one game's tree (tests / tools).
// nodesOut [maxNodes][24] u32, edgesOut [maxNodes][P][3] u32 (child bfs index, edge visits, move).
// SIDES (per-side match settings): word 21 follows the setting of the side whose search built the tree.
template <bool SIDES>
KC_D void gameTreeBody(const SearchDev& d, int g, int maxNodes, uint32_t* nodesOut, uint32_t* edgesOut,
                       int32_t* count) {
  if(threadIdx.x != 0)
    return;
  const GameDev& s = d.games[g];
  const Node* NS = d.nodes + (size_t)g * d.cap;
  if(s.rootIdx < 0) {
    *count = 0;
    return;
  }
  [[maybe_unused]] int32_t sideOn = 0;
  if constexpr(SIDES)
    sideOn = sideOf(d, g, s) ? d.unc1.on : d.unc.on;
  // canonical index map kept in nodesOut word 23 of each discovered node: store original idx
  int n = 0;
  int head = 0;
  nodesOut[23] = (uint32_t)s.rootIdx;
  n = 1;
  while(head < n && head < maxNodes) {
    const int idx = (int)nodesOut[(size_t)head * 24 + 23];
    const Node& x = NS[idx];
    uint32_t* o = nodesOut + (size_t)head * 24;
    o[0] = x.visits;
    o[1] = f2u(x.weightSum);
    o[2] = f2u(x.weightSqSum);
    o[3] = f2u(x.utilityAvg);
    o[4] = f2u(x.utilitySqAvg);
    o[5] = f2u(x.winLossAvg);
    o[6] = f2u(x.nnWin);
    o[7] = f2u(x.nnLoss);
    o[8] = f2u(x.lastSvbDelta);
    o[9] = f2u(x.lastSvbWeight);
    o[10] = (uint32_t)x.numChildren | ((uint32_t)x.nextPla << 16) | ((uint32_t)x.flags << 24);
    const uint64_t* nk = d.nodeKey + ((size_t)g * d.cap + idx) * 2;
    o[11] = (uint32_t)nk[0];
    o[12] = (uint32_t)(nk[0] >> 32);
    o[13] = (uint32_t)nk[1];
    o[14] = (uint32_t)(nk[1] >> 32);
    uint64_t sk = 0;
    int64_t sd = 0, sw = 0;
    if(x.svbEntry >= 0) {
      size_t e = ((size_t)g * 2 + s.svbSel) * d.svbCap + x.svbEntry;
      sk = d.svbKey[e];
      sd = d.svbD[e];
      sw = d.svbW[e];
    }
    o[15] = (uint32_t)sk;
    o[16] = (uint32_t)(sk >> 32);
    o[17] = (uint32_t)(uint64_t)sd;
    o[18] = (uint32_t)((uint64_t)sd >> 32);
    o[19] = (uint32_t)(uint64_t)sw;
    o[20] = (uint32_t)((uint64_t)sw >> 32);
    // the node's own evaluation weight with uncertainty weighting on (off: 0, as before)
    o[21] = (SIDES ? sideOn : d.unc.on) ? f2u(x.nnWeight) : 0u;
    o[22] = 0;
    const NodeEdges E{d.edges + ((size_t)g * d.cap + idx) * INLINE_EDGES,
                      d.edgePool + ((size_t)g * 2 + d.games[g].edgeSel) * d.edgePoolCap + x.edgeBase};
    for(int i = 0; i < x.numChildren; i++) {
      const int c = (int)E[i].child;
      int ci = -1;
      for(int q = 0; q < n; q++)
        if((int)nodesOut[(size_t)q * 24 + 23] == c) {
          ci = q;
          break;
        }
      if(ci < 0 && n < maxNodes) {
        nodesOut[(size_t)n * 24 + 23] = (uint32_t)c;
        ci = n++;
      }
      uint32_t* eo = edgesOut + ((size_t)head * d.P + i) * 3;
      eo[0] = (uint32_t)ci;
      eo[1] = E[i].visits;
      eo[2] = E[i].move;
    }
    head++;
  }
  // replace word 23 (original index) by 0 so the export is index independent
  for(int q = 0; q < n; q++)
    nodesOut[(size_t)q * 24 + 23] = 0;
  *count = n;
}

__global__ void kGameTree(const SearchDev* __restrict__ dp, int g, int maxNodes, uint32_t* nodesOut,
                          uint32_t* edgesOut, int32_t* count) {
  gameTreeBody<false>(*dp, g, maxNodes, nodesOut, edgesOut, count);
}
// The same export once more for an engine with per-side match settings (any other returns at
// once): launchGameTree has the device copy of SearchDev only, and kGameTree stays as it is.
__global__ void kGameTreeSides(const SearchDev* __restrict__ dp, int g, int maxNodes, uint32_t* nodesOut,
                               uint32_t* edgesOut, int32_t* count) {
  if(!dp->matchPerSide)
    return;
  gameTreeBody<true>(*dp, g, maxNodes, nodesOut, edgesOut, count);
}

// The priors beside kGameTree's export, in its breadth-first node order: priorsOut [maxNodes][P]
// f32 bits, each node's child priors (Edge::prior) in slot order, and nextOut [maxNodes][2], its
// cached next expansion (nextPrior bits, nextPos).  order [maxNodes]: scratch for the index map.
__global__ void kGameTreePriors(const SearchDev* __restrict__ dp, int g, int maxNodes, uint32_t* priorsOut,
                                uint32_t* nextOut, int32_t* order, int32_t* count) {
  if(threadIdx.x != 0)
    return;
  const SearchDev& d = *dp;
  const GameDev& s = d.games[g];
  const Node* NS = d.nodes + (size_t)g * d.cap;
  if(s.rootIdx < 0) {
    *count = 0;
    return;
  }
  int n = 1, head = 0;
  order[0] = s.rootIdx;
  while(head < n && head < maxNodes) {
    const int idx = order[head];
    const Node& x = NS[idx];
    nextOut[2 * (size_t)head] = f2u(x.nextPrior);
    nextOut[2 * (size_t)head + 1] = (uint32_t)x.nextPos;
    const NodeEdges E{d.edges + ((size_t)g * d.cap + idx) * INLINE_EDGES,
                      d.edgePool + ((size_t)g * 2 + s.edgeSel) * d.edgePoolCap + x.edgeBase};
    for(int i = 0; i < x.numChildren; i++) {
      const int c = (int)E[i].child;
      int ci = -1;
      for(int q = 0; q < n; q++)
        if(order[q] == c) {
          ci = q;
          break;
        }
      if(ci < 0 && n < maxNodes)
        order[n++] = c;
      priorsOut[(size_t)head * d.P + i] = f2u(E[i].prior);
    }
    head++;
  }
  *count = n;
}

// ---------------------------------------------------------------------------
// Position analysis (DESIGN.md "Analysis").  A slot holds one query or is idle.  An idle slot
// stands in PH_COMMIT with no leaf and no commit-list entry: kSelect gives it no network row
// and kBackup returns at once, so the round kernels run unchanged.  A search that reaches its
// visit limit is listed for the commit like a self-play move; kAnalysisReport takes kCommit's
// place, writes the result and refills the slot from the query ring.

// The next queued query's ring entry, or -1 (uniform).  The submitted count is written by the
// host between kernels only.
KC_D int popQuery(const SearchDev& d, int lane) {
  int q = -1;
  if(lane == 0) {
    unsigned long long* c = d.aCtr;
    const unsigned long long sub = c[AC_SUBMITTED];
    unsigned long long h = atomicAdd(&c[AC_POPPED], 0ull);
    while(h < sub) {
      const unsigned long long prev = atomicCAS(&c[AC_POPPED], h, h + 1ull);
      if(prev == h) {
        q = (int)(h % (unsigned long long)d.aCap);
        break;
      }
      h = prev;
    }
  }
  return bcastLane(q, 0);
}

// The ring entry of the next result (uniform).  Results outstanding never exceed aCap: every
// result answers a submitted query, and the host submits no more than aCap undrained ones.
KC_D int newResult(const SearchDev& d, int lane) {
  int r = 0;
  if(lane == 0)
    r = (int)(atomicAdd(&d.aCtr[AC_RESULTS], 1ull) % (unsigned long long)d.aCap);
  return bcastLane(r, 0);
}

// The bits 1..7 any lane has set (uniform).
KC_D uint32_t waveOrSyms(uint32_t x) {
  uint32_t r = 0;
#pragma unroll
  for(int s = 1; s < 8; s++)
    r |= ballot((x >> s) & 1u) != 0 ? 1u << s : 0u;
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
}

// The mask of the replayed position s.root under ring entry qi's restriction (rootmask.h, the
// rule coffee_root_mask runs on the host): the words into the slot's rootMask row, the used
// symmetries and the number of masked legal moves into syms / masked.  Returns the number of
// legal moves left unmasked.  Lane l takes the cells and positions l, l + 64, ...; every
// result is uniform.  Out of line like rareLeaf (arguments by value, the game's LDS copy
// through a pointer between fences).
// Returns the used symmetries (bits 0-7), the masked legal moves (bits 8-16) and the legal
// moves left unmasked (bits 17-25).
template <bool W1>
__device__ __noinline__ uint32_t rootMaskWave(const SearchDev* dp, const DTables* Tp, int g, const GameDev* gs, int qi) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const SearchDev& d = *uniformConst(dp);
  const DTables& T = *uniformConst(Tp);
  const GameDev& s = *uniformPtr(gs);
  g = __builtin_amdgcn_readfirstlane(g);
  qi = __builtin_amdgcn_readfirstlane(qi);
  GV v(d, T, g);
  const int A = d.A, P = d.P, W = (P + 31) >> 5;
  __shared__ uint32_t avoidW[RM_WORDS];
  const RootGeom rg{T.X, T.Y, A, P, &T.symCell[0][0], &T.symDir[0][0]};
  RootPos rp;
  rp.stones[0] = s.root.stones[0].lo;
  rp.stones[1] = s.root.stones[0].hi;
  rp.stones[2] = s.root.stones[1].lo;
  rp.stones[3] = s.root.stones[1].hi;
#pragma unroll
  for(int k = 0; k < 5; k++) {
    rp.histCell[k] = hCell(s.root, k);
    rp.histDir[k] = hDir(s.root, k);
  }
  uint32_t used = rmGeomSyms(rg);
  used &= ~rmHistoryBroken(rg, rp, used);
  used = (uint32_t)__builtin_amdgcn_readfirstlane((int)used);
  used &= ~waveOrSyms(rmStonesBroken(rg, rp, used, v.lane, 64));
  const coffee_analysis_restrict* rq = d.aRestrict + qi;
  const int mode = __builtin_amdgcn_readfirstlane((int)rq->mode);
  const bool have = mode == RM_AVOID || mode == RM_ALLOW;
  if(have) {
    // (every lane writes the same words)
    uint32_t qw[RM_QUERY_WORDS];
#pragma unroll
    for(int w = 0; w < RM_QUERY_WORDS; w++)
      qw[w] = rq->avoid[w];
    rmAvoidWords(P, qw, mode, avoidW);
    waveSync();
    used &= ~waveOrSyms(rmAvoidBroken(rg, avoidW, used, v.lane, 64));
  }
  uint32_t* mk = d.rootMask + (size_t)v.g * W;
  const bool prune = d.aPrune != 0;
  int left = 0, masked = 0;
  for(int base = 0; base < P; base += 64) {
    const int p = base + v.lane;
    const bool legal = p < P && isLegal<W1>(T, s.root, p % A, p / A);
    const bool m = p < P && rmMasked(rg, have ? avoidW : nullptr, used, prune, p, legal);
    const uint64_t bm = ballot(m), bl = ballot(legal);
    masked += __popcll(bm & bl);
    left += __popcll(bl & ~bm);
    if(v.lane == 0) {
      mk[base >> 5] = (uint32_t)bm;
      if((base >> 5) + 1 < W)
        mk[(base >> 5) + 1] = (uint32_t)(bm >> 32);
    }
  }
  waveSync();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  return used | ((uint32_t)masked << 8) | ((uint32_t)left << 17);
}

// Gives the slot the next queued query, or leaves it idle.  A query's moves are replayed from
// the empty board with the device rules, each checked before it is played; an illegal move, a
// move list that ends the game and a position without a legal move are answered at once (no
// search, GameDev::err untouched) and the next query is tried.  Otherwise the slot starts a
// fresh search the way startForkGame starts a forked game: stream seeded by startGame's
// formula from (seed, stream, game_num), game hashes from its first two draws, cleared tables,
// the replayed moves as unsearched turn records.  s: the slot's LDS copy (stored by the caller).
//
// One query per call of analysisRefillOne, which runs out of line like rareLeaf (arguments by
// value, the game's LDS copy through a pointer between fences) and returns REFILL_IDLE (nothing
// queued: the slot is idle), REFILL_LOADED or REFILL_ANSWERED (answered without a search: the
// caller tries the next query).  Every query's replay thus starts from the function's entry,
// with every lane active for its wave-wide rules, whatever path answered the query before it.
enum { REFILL_IDLE = 0, REFILL_LOADED = 1, REFILL_ANSWERED = 2 };
template <bool W1>
__device__ __noinline__ int analysisRefillOne(const SearchDev* dp, const DTables* Tp, int g, GameDev* gs) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const SearchDev& d = *uniformConst(dp);
  GameDev& s = *uniformPtr(gs);
  g = __builtin_amdgcn_readfirstlane(g);
  GV v(d, *uniformConst(Tp), g);
  bindGame<false>(v, s);
  const int A = d.A, P = d.P;
  {
    const int qi = popQuery(d, v.lane);
    if(qi < 0) {
      s.phase = PH_COMMIT;
      s.leafKind = LEAF_NONE;
      if(v.lane == 0)
        d.aSlot[v.g].busy = 0;
      waveSync();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      return REFILL_IDLE;
    }
    const coffee_analysis_query* q = d.aQuery + qi;
    const uint64_t id = q->id;
    // the host checked both ranges (coffee_analysis_submit); nothing here indexes past them anyway
    // every decision of the replay is taken on scalar values (each lane computes the same ones,
    // which the compiler cannot know): the branches stay scalar and every lane stays active
    // for the wave-wide rules (playMoveWave's ballot)
    const int nm = __builtin_amdgcn_readfirstlane(min(max((int)q->num_moves, 0), min(A, COFFEE_ANALYSIS_MAX_MOVES)));
    boardInit(v.T, s.root);
    waveSync();
    int bad = -1;
    for(int t = 0; t < nm; t++) {
      const int mv = __builtin_amdgcn_readfirstlane((int)q->moves[t]);
      bool ok = __builtin_amdgcn_readfirstlane(s.root.finished) == 0 && mv < P;
      if(ok)
        ok = __builtin_amdgcn_readfirstlane((int)isLegal<W1>(v.T, s.root, mv % A, mv / A)) != 0;
      if(!ok) {
        bad = t;
        break;
      }
      playMoveWave<W1>(v.T, s.root, mv % A, mv / A);
      waveSync();
    }
    const int over = __builtin_amdgcn_readfirstlane(s.root.finished);
    if(bad >= 0 || over != 0) {
      const int ri = newResult(d, v.lane);
      if(v.lane == 0) {
        coffee_analysis_result r;
        memset(&r, 0, sizeof(r));
        r.id = id;
        if(bad >= 0) {
          r.status = COFFEE_ANALYSIS_ILLEGAL_MOVE;
          r.info = bad;
        } else if(s.root.winner == 0 && s.root.turn < A) {
          r.status = COFFEE_ANALYSIS_NO_LEGAL_MOVE;
        } else {
          r.status = COFFEE_ANALYSIS_GAME_OVER;
          r.info = s.root.winner;
        }
        r.turn = s.root.turn;
        r.pla = s.root.pla;
        d.aRes[ri] = r;
        d.aRootInfo[ri] = coffee_analysis_root_info{0u, 0};
        atomicAdd(&d.aCtr[AC_LOADED], 1ull);
        atomicAdd(&d.aCtr[AC_FINISHED], 1ull);
        atomicAdd(&d.aCtr[AC_REJECTED], 1ull);
      }
      waveSync();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      return REFILL_ANSWERED;
    }
    // the root restrictions, once per query; a mask that leaves no legal move is answered at
    // once like the cases above (symmetry pruning alone always leaves each orbit's survivor)
    const uint32_t rm = (uint32_t)__builtin_amdgcn_readfirstlane((int)rootMaskWave<W1>(&d, &v.T, v.g, &s, qi));
    const uint32_t syms = rm & 0xFFu;
    const int masked = (int)((rm >> 8) & 0x1FFu), left = (int)(rm >> 17);
    if(left == 0) {
      const int ri = newResult(d, v.lane);
      if(v.lane == 0) {
        coffee_analysis_result r;
        memset(&r, 0, sizeof(r));
        r.id = id;
        r.status = COFFEE_ANALYSIS_NO_ALLOWED_MOVE;
        r.turn = s.root.turn;
        r.pla = s.root.pla;
        d.aRes[ri] = r;
        d.aRootInfo[ri] = coffee_analysis_root_info{syms, masked};
        atomicAdd(&d.aCtr[AC_LOADED], 1ull);
        atomicAdd(&d.aCtr[AC_FINISHED], 1ull);
        atomicAdd(&d.aCtr[AC_REJECTED], 1ull);
      }
      waveSync();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      return REFILL_ANSWERED;
    }
    s.rngSeed = mix64(d.seed ^ mix64(((uint64_t)q->stream << 32) | (uint32_t)q->game_num));
    s.gameNum = (int32_t)q->game_num;
    s.startGen = *d.modelGen;
    clearTables(v, s);
    TurnRec* tr = v.turns();
    for(int t = v.lane; t < nm; t += 64) {
      const int mv = (int)q->moves[t];
      TurnRec rec;
      memset(&rec, 0, sizeof(rec));
      rec.gen = (uint8_t)*d.modelGen;
      rec.cell = (int8_t)(mv % A);
      rec.dir = (int8_t)(mv / A);
      tr[t] = rec;
    }
    s.numTurns = nm;
    s.startTurn = nm;
    s.moves = (uint64_t)nm;
    s.initLeft = 0;
    s.gameMode = 0;
    s.sideCount = 0;
    s.sideNext = 0;
    s.sideMode = 0;
    s.startDelay = 0;
    DRng rng{s.rngSeed, 0};
    s.gameHash0 = rng.next();
    s.gameHash1 = rng.next();
    const uint64_t ctr = q->rng_counter;
    s.rngCtr = ctr != 0 ? ctr : rng.ctr;
    const int mvis = (int)q->max_visits;
    s.visitLimit = min(mvis > 0 ? mvis : d.sp.maxVisits, d.cap - 4);
    s.moveWeight = 1.0f;
    s.noNoise = 0;
    s.phase = PH_ROOTEVAL;
    s.rootK = 0;
    s.leafKind = LEAF_NONE;
    if(v.lane == 0) {
      d.aSlot[v.g].id = id;
      d.aSlot[v.g].busy = 1;
      d.aSlot[v.g].syms = syms;
      d.aSlot[v.g].numMasked = masked;
      atomicAdd(&d.aCtr[AC_LOADED], 1ull);
    }
    waveSync();
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  return REFILL_LOADED;
}
template <bool W1>
KC_D void analysisRefill(const GV& v, GameDev& s) {
  while(__builtin_amdgcn_readfirstlane(analysisRefillOne<W1>(&v.d, &v.T, v.g, &s)) == REFILL_ANSWERED) {
  }
  waveSync();
}

// Every slot idle (after kInit started a game in each).
__global__ void kAnalysisInit(const SearchDev* __restrict__ dp) {
  const SearchDev& d = *dp;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if(g >= d.G)
    return;
  d.games[g].phase = PH_COMMIT;
  d.games[g].leafKind = LEAF_NONE;
  d.aSlot[g].busy = 0;
}

__global__ void kAnalysisSubmitted(const SearchDev* __restrict__ dp, unsigned long long submitted) {
  dp->aCtr[AC_SUBMITTED] = submitted;
}

// One wave per slot: an idle slot takes the next queued query (launched with every report,
// and by every step before its first round, after the host's submissions).
template <int NI>
__global__ void __launch_bounds__(64) kAnalysisLoad(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  // (constant views, as in kBackup: uniform reads stay scalar loads after the kernel's own stores)
  const SearchDev& d = *uniformConst(dp);
  const DTables& T = *uniformConst(Tp);
  const int g = blockIdx.x;
  if(g >= d.G || d.aSlot[g].busy != 0)
    return;
  if(d.aCtr[AC_POPPED] >= d.aCtr[AC_SUBMITTED])  // nothing queued (a later pop re-checks atomically)
    return;
  __shared__ GameDev s;
  GV v(d, T, g);
  loadGame(v, s);
  analysisRefill<W1_OF<NI>>(v, s);
  waveSync();
  storeGame(v, s);
}

// One wave per finished search, over the commit list (where self-play runs kCommit): the
// result header from the root's record, one record per root child in child-slot order -- lane
// l holds children l, l + 64, ... as everywhere -- and the slot's refill.  Per child: the
// edge and the child's record as stored (white's perspective), the root's NN policy of the
// move before temperature and noise, lcbAndRadius, the play-selection value at the settings
// the move choice uses (no pruning when chosen_move_subtract / _prune are 0), its rank, and
// the principal variation: each lane walks its own children's lines, at every node to the
// child with the most edge visits (ties: lower slot), until a node without children or a
// terminal node.  The tree is not changed.
template <int NI, bool EXPL = false>
__global__ void __launch_bounds__(64) kAnalysisReport(const SearchDev* __restrict__ dp, const DTables* __restrict__ Tp) {
  // (constant views, as in kBackup: uniform reads stay scalar loads after the kernel's own stores)
  const SearchDev& d = *uniformConst(dp);
  const DTables& T = *uniformConst(Tp);
  if((int)blockIdx.x >= *d.commitCount)
    return;
  const int g = d.commitList[blockIdx.x];
  __shared__ int posv[MAX_P];
  __shared__ float vals[MAX_P];
  __shared__ GameDev s;
  // a list entry is reported once: the list outlives its commit until the next kSelect
  // empties it, and the launch also runs at the start of a step
  if(d.aSlot[g].busy == 0 || d.games[g].phase != PH_COMMIT)
    return;
  GV v(d, T, g);
  loadGame(v, s);
  const SP& sp = d.sp;
  const Node* NS = v.nodes();
  const Node root = NS[s.rootIdx];
  const int k = root.numChildren, pla = root.nextPla;
  // (a root without children gets the direct policy moves here: not children, not reported)
  playSelectionValues<NI, EXPL>(v, sp, s, 0.0f, true, posv, vals, sp.useLcb != 0);
  const int ri = newResult(d, v.lane);
  const NodeEdges E = v.edges(s.rootIdx, root.edgeBase);
  const float* rp = v.pol(s.rootIdx);
  const Edge* pool = v.edgePool();
  const int maxPv = min(d.aMaxPv, COFFEE_ANALYSIS_MAX_PV);
  coffee_analysis_move* out = d.aMoves + (size_t)ri * d.P;
#pragma unroll
  for(int j = 0; j < NI; j++) {
    const int i = v.lane + 64 * j;
    if(i >= k)
      continue;
    const Edge e = E[i];
    const Node c = NS[e.child];
    coffee_analysis_move* m = out + i;
    m->move = (int32_t)e.move;
    m->edge_visits = e.visits;
    m->visits = c.visits;
    m->weight_sum = c.weightSum;
    m->utility_avg = c.utilityAvg;
    m->win_loss_avg = c.winLossAvg;
    m->prior = rp[e.move];
    float lcb, radius;
    lcbAndRadius(sp, pla, c.visits, c.weightSum, c.weightSqSum, c.utilityAvg, c.utilitySqAvg, e.visits, lcb, radius);
    m->lcb = lcb;
    m->radius = radius;
    const float val = vals[i];
    m->play_selection_value = val;
    int order = 0;
    for(int o = 0; o < k; o++) {
      const float ov = vals[o];
      order += (ov > val || (ov == val && o < i)) ? 1 : 0;
    }
    m->order = order;
    int len = 0;
    uint32_t node = e.child;
    uint32_t mv = e.move;
    while(len < maxPv) {
      m->pv[len++] = (uint16_t)mv;
      const Node& n = NS[node];
      const int nk = n.numChildren;
      if(nk == 0 || (n.flags & 2))
        break;
      const Edge* inl = v.inlineEdges((int)node);
      const Edge* pl = pool + n.edgeBase;
      uint32_t bestVis = 0, bestChild = 0, bestMove = 0;
      for(int o = 0; o < nk; o++) {
        const Edge ce = o < INLINE_EDGES ? inl[o] : pl[o - INLINE_EDGES];
        if(o == 0 || ce.visits > bestVis) {
          bestVis = ce.visits;
          bestChild = ce.child;
          bestMove = ce.move;
        }
      }
      node = bestChild;
      mv = bestMove;
    }
    m->pv_len = len;
    for(int t = len; t < COFFEE_ANALYSIS_MAX_PV; t++)
      m->pv[t] = 0;
  }
  if(v.lane == 0) {
    coffee_analysis_result r;
    r.id = d.aSlot[g].id;
    r.status = COFFEE_ANALYSIS_OK;
    r.info = 0;
    r.turn = s.root.turn;
    r.pla = s.root.pla;
    r.visits = root.visits;
    r.weight_sum = root.weightSum;
    r.utility_avg = root.utilityAvg;
    r.win_loss_avg = root.winLossAvg;
    r.nn_win = root.nnWin;
    r.nn_loss = root.nnLoss;
    r.num_children = k;
    r.pad = 0;
    d.aRes[ri] = r;
    d.aRootInfo[ri] = coffee_analysis_root_info{d.aSlot[g].syms, d.aSlot[g].numMasked};
    atomicAdd(&d.aCtr[AC_FINISHED], 1ull);
  }
  if(d.aPolicy.p != nullptr) {  // the root's network policy as stored (no temperature, noise or mask)
    float* po = d.aPolicy + (size_t)ri * d.P;
    for(int p = v.lane; p < d.P; p += 64)
      po[p] = rp[p];
  }
  waveSync();
  analysisRefill<W1_OF<NI>>(v, s);
  waveSync();
  storeGame(v, s);
}

// ---------------------------------------------------------------------------
static int laneItems(int P) { return P <= 128 ? 2 : (P <= 256 ? 4 : 7); }

// The launchers' choice of a kernel instantiation: f is a generic lambda that takes the
// choice as a type and names the kernel once -- byItems the engine's items per lane
// (f(std::integral_constant<int, NI>{}), NI = laneItems(P)), byFlag a template flag
// (f(std::true_type{}) or f(std::false_type{})).
template <class F>
static void byItems(int P, F f) {
  switch(laneItems(P)) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 7>{}); break;
  }
}
template <class F>
static void byFlag(bool b, F f) {
  if(b)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// ---------------------------------------------------------------------------
// Row staging for device-resident gathers (coffee_selfplay_stage_rows): one wave per
// row packs the row's six arrays into one contiguous record (rows.py FIELDS: bin u8
// [15][pb], glob f32, pol i16 [2][P], gt f32 [64], val i8 [5][A], meta i32 [4]), so a
// rank's rows leave as one device block for the RCCL gather.
__global__ void __launch_bounds__(256) kStageRows(const SearchDev* __restrict__ dp, uint8_t* __restrict__ dst,
                                                  int rb) {
  const SearchDev& d = *dp;
  const int A = d.A, P = d.P, pb = (A + 7) / 8;
  const unsigned long long n = *d.rCount;
  const int lane = threadIdx.x & 63;
  const int sz[6] = {NUM_SPATIAL * pb, 4, 4 * P, 256, 5 * A, 16};
  for(unsigned long long r = blockIdx.x * 4ull + (threadIdx.x >> 6); r < n; r += gridDim.x * 4ull) {
    const uint8_t* src[6] = {d.rBin + r * sz[0], reinterpret_cast<const uint8_t*>(d.rGlob + r),
                             reinterpret_cast<const uint8_t*>(d.rPol + r * 2 * P),
                             reinterpret_cast<const uint8_t*>(d.rGt + r * 64), reinterpret_cast<const uint8_t*>((const int8_t*)d.rVal) + r * sz[4],
                             reinterpret_cast<const uint8_t*>(d.rMeta + r * 4)};
    uint8_t* o = dst + r * (unsigned long long)rb;
#pragma unroll
    for(int f = 0; f < 6; f++) {
      for(int i = lane; i < sz[f]; i += 64)
        o[i] = src[f][i];
      o += sz[f];
    }
  }
}

__global__ void kStageDone(const SearchDev* __restrict__ dp, int discardGames) {
  const SearchDev& d = *dp;
  *d.rStaged += *d.rCount;
  *d.rCount = 0;
  if(discardGames)
    *d.gCount = 0;
}

void launchStageRows(const SearchDev& d, const SearchDev* dd, uint8_t* dst, unsigned long long* countOut,
                     bool discardGames, hipStream_t st) {
  hipLaunchKernelGGL(kStageRows, dim3(1024), dim3(256), 0, st, dd, dst, rowBytes(d.A));
  KC_HIP(hipGetLastError());
  KC_HIP(hipMemcpyAsync(countOut, d.rCount, 8, hipMemcpyDeviceToHost, st));
  hipLaunchKernelGGL(kStageDone, dim3(1), dim3(1), 0, st, dd, discardGames ? 1 : 0);
  KC_HIP(hipGetLastError());
}

void launchStartPosCheck(const DTables* T, int P, const coffee_start_position* samples, int n, int32_t* status,
                         int32_t* info, hipStream_t st) {
  if(n <= 0)
    return;
  byItems(P, [&](auto ni) {
    hipLaunchKernelGGL(kStartPosCheck<ni()>, dim3(n), dim3(64), 0, st, T, samples, n, status, info);
  });
  KC_HIP(hipGetLastError());
}

void launchSelfplayInit(const SearchDev& d, const SearchDev* dd, hipStream_t st) {
  hipLaunchKernelGGL(kInit, dim3(d.G), dim3(64), 0, st, dd, d.T);
  KC_HIP(hipGetLastError());
  if(d.matchMode && d.matchPerSide) {
    hipLaunchKernelGGL(kMatchSideLimits, dim3((d.G + 255) / 256), dim3(256), 0, st, dd);
    KC_HIP(hipGetLastError());
  }
  if(d.analysisMode) {
    hipLaunchKernelGGL(kAnalysisInit, dim3((d.G + 255) / 256), dim3(256), 0, st, dd);
    KC_HIP(hipGetLastError());
  }
}

// 256 threads (one wave per SIMD) while each wave keeps at most CP_CH chunks of 64 games: a workgroup
// that small fits beside a network workgroup of the other game group on its CU (1024
// threads need 4 waves per SIMD) and does not wait for a free one.
void launchCompact(const SearchDev& d, const SearchDev* dd, hipStream_t st, bool accumulate, bool resolve) {
  const int nt = d.G <= 4 * 64 * CP_CH ? 256 : 1024;  // 1024 only past 8192 games per engine
  const DTables* T = d.T;
  const int a = accumulate ? 1 : 0;
  if(d.wideK > 1)
    hipLaunchKernelGGL(kCompactWide, dim3(1), dim3(d.G * d.wideK <= 256 ? 256 : 1024), 0, st, dd, a);
  else if(d.matchMode)
    hipLaunchKernelGGL((kCompact<2, false, true>), dim3(1), dim3(nt), 0, st, dd, T, a);
  else if(!resolve)
    hipLaunchKernelGGL((kCompact<2, false>), dim3(1), dim3(nt), 0, st, dd, T, a);
  else
    byItems(d.P, [&](auto ni) { hipLaunchKernelGGL((kCompact<ni(), true>), dim3(1), dim3(nt), 0, st, dd, T, a); });
  KC_HIP(hipGetLastError());
}

// A launch, with start/end events recorded by the dispatch itself when given.
template <class K, class... Args>
static void launchEv(K kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t st, hipEvent_t e0, hipEvent_t e1,
                     Args... args) {
  if(e0)
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, e0, e1, 0, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// Whether the engine's searches carry variance-scaled exploration or noise pruning (explore.h;
// DESIGN.md 8g): the launchers then take the EXPL instantiations, every other engine the ones
// without them, which hold no trace of either mechanism.
static bool explLaunch(const SearchDev& d) {
  return explOn(d.ex) || explOn(d.ex1) || rootSearchOn(d.rs) || rootSearchOn(d.rs1);
}

void launchSelect(const SearchDev& d, const SearchDev* dd, hipStream_t st, hipEvent_t e0, hipEvent_t e1,
                  bool resetCommit) {
  const int rc = resetCommit ? 1 : 0;
  if(d.wideK > 1) {  // parallel playouts: an analysis engine's setting
    byItems(d.P, [&](auto ni) {
      byFlag(explLaunch(d), [&](auto e) {
        launchEv(kSelectWide<ni(), e()>, dim3(d.G), dim3(64), 0, st, e0, e1, dd, d.T, rc);
      });
    });
    KC_HIP(hipGetLastError());
    return;
  }
  byItems(d.P, [&](auto ni) {
    byFlag(d.matchMode, [&](auto m) {
      byFlag(explLaunch(d), [&](auto e) {
        launchEv(kSelect<ni(), m(), e()>, dim3(d.G), dim3(64), 0, st, e0, e1, dd, d.T, rc);
      });
    });
  });
  KC_HIP(hipGetLastError());
}

void launchBackup(const SearchDev& d, const SearchDev* dd, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if(d.wideK > 1) {
    byItems(d.P, [&](auto ni) {
      byFlag(explLaunch(d), [&](auto e) {
        launchEv(kBackupWide<ni(), e()>, dim3(d.G), dim3(64), 0, st, e0, e1, dd, d.T);
      });
    });
    KC_HIP(hipGetLastError());
    return;
  }
  byItems(d.P, [&](auto ni) {
    byFlag(d.matchMode, [&](auto m) {
      byFlag(explLaunch(d), [&](auto e) {
        launchEv(kBackup<ni(), m(), e()>, dim3(d.G), dim3(64), 0, st, e0, e1, dd, d.T);
      });
    });
  });
  KC_HIP(hipGetLastError());
}

void launchBackupSelect(const SearchDev& d, const SearchDev* dd, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  byItems(d.P, [&](auto ni) {
    byFlag(explLaunch(d), [&](auto e) {
      launchEv(kBackupSelect<ni(), e()>, dim3(d.G), dim3(64), 0, st, e0, e1, dd, d.T);
    });
  });
  KC_HIP(hipGetLastError());
}

void launchResolve(const SearchDev& d, const SearchDev* dd, hipStream_t st) {
  byItems(d.P, [&](auto ni) { hipLaunchKernelGGL(kResolve<ni()>, dim3(RESOLVE_GRID), dim3(64), 0, st, dd, d.T); });
  KC_HIP(hipGetLastError());
}

void launchCommit(const SearchDev& d, const SearchDev* dd, hipStream_t st) {
  if(d.analysisMode) {
    // nothing is played: the finished searches are reported and their slots refilled, then
    // the idle slots take the queries submitted so far
    hipLaunchKernelGGL(kAnalysisSubmitted, dim3(1), dim3(1), 0, st, dd, d.aSubmitted);
    KC_HIP(hipGetLastError());
    byItems(d.P, [&](auto ni) {
      byFlag(explLaunch(d), [&](auto e) {
        hipLaunchKernelGGL((kAnalysisReport<ni(), e()>), dim3(d.G), dim3(64), 0, st, dd, d.T);
      });
      hipLaunchKernelGGL(kAnalysisLoad<ni()>, dim3(d.G), dim3(64), 0, st, dd, d.T);
    });
    KC_HIP(hipGetLastError());
    return;
  }
  const size_t lds = commitLdsBytes(d.cap);
  byItems(d.P, [&](auto ni) {
    byFlag(d.matchMode, [&](auto m) {
      byFlag(explLaunch(d), [&](auto e) {
        hipLaunchKernelGGL((kCommit<ni(), m(), e()>), dim3(d.G), dim3(64), lds, st, dd, d.T);
      });
    });
  });
  KC_HIP(hipGetLastError());
  if(!d.matchMode) {  // match play writes no training rows
    hipLaunchKernelGGL(kRows, dim3(d.G), dim3(64 * ROWS_WAVES), 0, st, dd, d.T);
    KC_HIP(hipGetLastError());
  }
  if(d.spN > 0) {  // a start-position table is set: the new games' turn records, after kRows
    hipLaunchKernelGGL(kStartPosTurns, dim3(d.G), dim3(64), 0, st, dd, d.T);
    KC_HIP(hipGetLastError());
  }
}

void launchVirtualLossCount(const SearchDev& d, const SearchDev* dd, unsigned long long* out, hipStream_t st) {
  KC_HIP(hipMemsetAsync(out, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(kVirtualLossCount, dim3(d.G), dim3(64), 0, st, dd, out);
  KC_HIP(hipGetLastError());
}

void launchGameTree(const SearchDev* dd, int slot, int maxNodes, uint32_t* nodesOut, uint32_t* edgesOut,
                    int32_t* count, hipStream_t st) {
  hipLaunchKernelGGL(kGameTree, dim3(1), dim3(64), 0, st, dd, slot, maxNodes, nodesOut, edgesOut, count);
  KC_HIP(hipGetLastError());
  hipLaunchKernelGGL(kGameTreeSides, dim3(1), dim3(64), 0, st, dd, slot, maxNodes, nodesOut, edgesOut, count);
  KC_HIP(hipGetLastError());
}

void launchGameTreePriors(const SearchDev* dd, int slot, int maxNodes, uint32_t* priorsOut, uint32_t* nextOut,
                          int32_t* order, int32_t* count, hipStream_t st) {
  hipLaunchKernelGGL(kGameTreePriors, dim3(1), dim3(64), 0, st, dd, slot, maxNodes, priorsOut, nextOut, order, count);
  KC_HIP(hipGetLastError());
}

}  // namespace kc
