// Start positions (reference GameInitializer startPoses, play.cpp:186-248 and
// :400-448): a share of the games starts from a sample of a table of move lists instead of
// the empty board.  The table's weights become 64-bit fixed-point cumulative thresholds on the
// host; a game's pick is an integer comparison of one raw draw against them, so host and
// device agree exactly and a large table loses nothing to float rounding.
// The same code on host and device (coffee_start_position_pick runs startPosDraw).
#pragma once
#include <cmath>

#include "detmath.h"

namespace kc {

// The stream of game `gameNum` of global slot `globalSlot` (startGame, startForkGame and
// analysisRefill seed their games with it).
KC_HD uint64_t gameStreamSeed(uint64_t seed, uint32_t globalSlot, uint32_t gameNum) {
  return mix64(seed ^ mix64(((uint64_t)globalSlot << 32) | gameNum));
}

// Thresholds of n samples with unnormalised probabilities exp(-numMoves * lambda) * weight
// (generateCumProbs play.cpp:121-133, initialTurnNumber 0), computed in double:
// cum[i] = floor(2^64 * (p_0 + .. + p_i) / sum), nondecreasing; from the last sample with
// positive probability on, 2^64 - 1.  A sample of probability 0 repeats its predecessor's
// threshold (0 for the first).  Returns false for a negative or non-finite weight or
// probability and for a table whose probabilities are all 0.
inline bool startPosThresholds(const float* weight, const int32_t* numMoves, int n, double lambda, uint64_t* cum) {
  if(n < 1)
    return false;
  double total = 0.0;
  int lastPositive = -1;
  for(int i = 0; i < n; i++) {
    const double w = (double)weight[i];
    if(!(w >= 0.0) || !std::isfinite(w))
      return false;
    const double p = std::exp(-(double)numMoves[i] * lambda) * w;
    if(!std::isfinite(p))
      return false;
    total += p;
    if(p > 0.0)
      lastPositive = i;
  }
  if(lastPositive < 0 || !std::isfinite(total) || !(total > 0.0))
    return false;
  double run = 0.0;
  for(int i = 0; i < n; i++) {
    run += std::exp(-(double)numMoves[i] * lambda) * (double)weight[i];
    const double frac = run / total;
    // frac < 1: frac * 2^64 is exact in double and below 2^64
    cum[i] = (i >= lastPositive || frac >= 1.0) ? ~0ULL : (uint64_t)std::ldexp(frac, 64);
  }
  return true;
}

// The sample of raw draw r: the first i with r < cum[i]; r = 2^64 - 1 takes the first i whose
// threshold is 2^64 - 1, the last sample with positive probability.  Binary search over the
// nondecreasing thresholds (cum[n-1] = 2^64 - 1, so the search always ends inside the table).
KC_HD int startPosIndex(const uint64_t* cum, int n, uint64_t r) {
  int lo = 0, hi = n - 1;
  while(lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint64_t c = cum[mid];
    if(r < c || c == ~0ULL)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// startGame's draws for the start position, on the game's stream after its two hash draws:
// none without a table or with prob 0; else u = uni(), and for u < prob one raw draw and the
// pick.  Returns the sample, or -1 for the empty board.
KC_HD int startPosDraw(DRng& rng, float prob, const uint64_t* cum, int n) {
  if(n <= 0 || cum == nullptr || !(prob > 0.0f))
    return -1;
  const float u = rng.uni();
  if(!(u < prob))
    return -1;
  return startPosIndex(cum, n, rng.next());
}

}  // namespace kc
