// Uncertainty weighting of playouts (reference useUncertainty,
// Search::computeWeightFromNNOutput searchupdatehelpers.cpp:98-120): an evaluation whose
// short-term error the net predicts to be large counts for less in every average above it.
// The same detmath.h sequences on host and device, so both agree bit for bit.
#pragma once
#include "detmath.h"

namespace kc {

// SearchDev's copy of coffee_uncertainty_params.
struct Unc {
  int32_t on;
  float coeff, exponent, maxWeight;
};

// Short-term win/loss error of an evaluation from its logit out[P+3] (nneval.cpp:789-793,
// model multiplier 0.25 desc.cpp:962).
KC_HD float stErrorOf(float logit) {
  const float h = 0.5f * logit;
  const float s = h > 40.0f ? h : dlog(1.0f + dexp(h));
  return sqrtf(s * s * 0.25f);
}

// The evaluation's weight (win/loss utility factor 1, no score term); 1 with the setting off.
KC_HD float uncWeightOf(const Unc& u, float err) {
  if(!u.on)
    return 1.0f;
  const float p = u.exponent == 1.0f ? err : (u.exponent == 0.5f ? sqrtf(err) : dpow(err, u.exponent));
  return u.coeff / (p + u.coeff / u.maxWeight);
}
// A terminal visit's weight (search.cpp:949-951).
KC_HD float uncTerminalWeight(const Unc& u) { return u.on ? u.maxWeight : 1.0f; }

}  // namespace kc
