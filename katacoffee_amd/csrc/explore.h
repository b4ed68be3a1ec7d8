// Variance-scaled exploration and noise pruning (reference
// cpuctUtilityStdevScale, getFpuValueForChildrenAssumeVisited searchexplorehelpers.cpp:256-277,
// and useNoisePruning, pruneNoiseWeight searchupdatehelpers.cpp:423-467).  f32 and the
// detmath.h sequences only, in the written operation order, so host and device agree bit for bit.
#pragma once
#include "detmath.h"

namespace kc {

// SearchDev's copy of coffee_exploration_params.
struct Expl {
  int32_t noisePruning;
  float pruneUtilityScale, pruningCap;
  float stdevPrior, stdevPriorWeight, stdevScale;
};

// Whether a search with these parameters differs from one without them (the launchers then
// pick the kernel instantiations that carry the two mechanisms).
KC_HD bool explOn(const Expl& e) { return e.noisePruning != 0 || e.stdevScale != 0.0f; }

// The factor on the exploration scaling from the spread of the parent's utility; exactly 1
// with scale 0.
KC_HD float exploreStdevFactor(const Expl& e, uint32_t visits, float weightSum, float utilityAvg, float utilitySqAvg) {
  if(e.stdevScale == 0.0f)
    return 1.0f;
  float stdev;
  if(visits <= 0u || weightSum <= 1.0f)
    stdev = e.stdevPrior;
  else {
    const float usq = utilityAvg * utilityAvg;
    const float usqA = utilitySqAvg < usq ? usq : utilitySqAvg;
    const float var =
        ((usq + e.stdevPrior * e.stdevPrior) * e.stdevPriorWeight + usqA * weightSum) / (e.stdevPriorWeight + weightSum - 1.0f) -
        usq;
    stdev = sqrtf(var < 0.0f ? 0.0f : var);
  }
  return 1.0f + e.stdevScale * (stdev / e.stdevPrior - 1.0f);
}

// The running sums of the noise-pruning scan over a node's good children in slot order.
struct PruneScan {
  float uSum, wSum, pSum;
};

// One child of the scan: its weight after pruning (old: its weight before, u: its utility from
// the parent's side, prior: the parent's prior of its move); the sums then include it.
KC_HD float pruneNoiseStep(const Expl& e, PruneScan& sc, float old, float u, float prior) {
  const float p = prior < 1e-30f ? 1e-30f : prior;
  float nw = old;
  if(sc.wSum > 0.0f && sc.pSum > 0.0f) {
    const float gap = sc.uSum / sc.wSum - u;
    if(gap > 0.0f) {
      const float lenient = 2.0f * ((sc.wSum * p) / sc.pSum);
      if(old > lenient) {
        float sub = (old - lenient) * (1.0f - dexp(-gap / e.pruneUtilityScale));
        if(sub > e.pruningCap)
          sub = e.pruningCap;
        nw = old - sub;
      }
    }
  }
  sc.uSum = sc.uSum + u * nw;
  sc.wSum = sc.wSum + nw;
  sc.pSum = sc.pSum + p;
  return nw;
}

// Whether the scan runs at all for numGood good children of total weight `total`.
KC_HD bool pruneNoiseApplies(int numGood, float total) { return numGood > 1 && total > 0.00001f; }

}  // namespace kc
