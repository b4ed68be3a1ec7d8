// Virtual losses of the parallel playouts of one search (reference
// numVirtualLossesPerThread, getExploreSelectionValueOfChild searchexplorehelpers.cpp:125-134).
// f32 only, in the written operation order, so host and device agree bit for bit.
#pragma once
#include "detmath.h"

namespace kc {

// Descents a searching slot may make in one round (coffee_analysis_set_search_threads).
constexpr int MAX_SEARCH_THREADS = 32;

// A child that `vl` unfinished playouts of this round have entered, as its parent's selection
// sees it: each of them counts as perThread visits that lost for the parent's mover (utilities
// span [-1, 1]: the loss is -1 with white to move at the parent, +1 with black).  u: the value
// the selection would use without them (the child's utilityAvg, or the first-play urgency of a
// child without visits), w: the child's weight.  vl == 0 leaves both as they are.
KC_HD void virtualLossAdjust(float perThread, uint32_t vl, int pla, float& u, float& w) {
  if(vl == 0u)
    return;
  const float lossU = pla == 2 ? -1.0f : 1.0f;
  const float vlw = (float)vl * perThread;
  const float frac = vlw / (vlw + fmaxf(0.25f, w));
  u = u + (lossU - u) * frac;
  w = w + vlw;
}

}  // namespace kc
