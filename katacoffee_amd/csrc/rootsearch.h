// Wide root noise and futile-visit pruning of the root's child selection (DESIGN.md §8h;
// reference maybeApplyWideRootNoise searchexplorehelpers.cpp:71-87, getExploreSelectionValueOfChild
// :136-172, getNewExploreSelectionValue :182-207, upperBoundVisitsLeft search.cpp:477-483).
// Both act at the root only and during search only.  f32 and the detmath.h sequences only, in
// the written operation order, so host and device agree bit for bit.
#pragma once
#include <cfloat>

#include "detmath.h"

namespace kc {

// SearchDev's copy of coffee_root_search_params.
struct RootSearch {
  float wide;  // wideRootNoise (0: off)
  float thr;   // futileVisitsThreshold (0: off)
};

// Whether a search with these parameters differs from one without them (the launchers then
// pick the kernel instantiations that carry the two rules).
KC_HD bool rootSearchOn(const RootSearch& r) { return r.wide > 0.0f || r.thr > 0.0f; }

// The selection value of a futile root move: below every other legal move's, above an illegal
// or masked move's -inf (the reference's -1e40 against -1e50, which f32 does not hold).
constexpr float FUTILE_VALUE = -FLT_MAX;

// Futile-visit pruning.  maxW: the largest child weight; wpv: the root's weight per visit;
// left: the visits the search still has.
KC_HD bool futileChild(float thr, float maxW, float wpv, float left, uint32_t edgeVisits, uint32_t childVisits, float w) {
  const float need = (thr * maxW) * (((float)edgeVisits + 1.0f) / (w + wpv));
  return (float)childVisits + left < need;
}
KC_HD bool futileNew(float thr, float maxW, float wpv, float left) {
  const float need = (thr * maxW) * (1.0f / wpv);
  return left < need;
}

// Wide root noise.  The draws of one root selection come from a stream of their own, a pure
// function of the game's stream seed, the root's turn and its visit count at the selection;
// each move then reads at its own policy position.  The game's main stream is not touched.
constexpr uint64_t WIDE_ROOT_TAG = 0x57494445524F4F54ULL;  // "WIDEROOT"
KC_HD uint64_t wideRootKey(uint64_t rngSeed, int32_t turn, uint32_t rootVisits) {
  return mix64(rngSeed ^ WIDE_ROOT_TAG ^ ((uint64_t)(uint32_t)turn << 32) ^ (uint64_t)rootVisits);
}
KC_HD float wideSmoothedPrior(float wide, float p) { return dpow(p, 1.0f / (4.0f * wide + 1.0f)); }
// The bonus on the utility from the mover's side for the move at policy position pos: with
// probability 1/2 wide * |gauss|, else 0.
KC_HD float wideBonus(float wide, uint64_t key, int pos) {
  DRng r{key, (uint64_t)pos << 8};
  const uint64_t coin = r.next() >> 63;
  return coin ? wide * fabsf(r.gauss()) : 0.0f;
}
// u with the bonus: the utility is white's, the bonus the mover's (pla 2: white to move).
KC_HD float wideUtility(float u, float bonus, int pla) { return pla == 2 ? u + bonus : u - bonus; }

}  // namespace kc
