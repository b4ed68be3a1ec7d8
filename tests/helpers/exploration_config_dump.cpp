// Prints what the config layer (cli_config.h, header-only) resolves a config file's exploration
// keys to: one line "use scale cap prior priorWeight stdevScale" for the plain keys (applyConfig,
// what selfplay / gatekeeper / analysis read) and one per bot of `katago match` (applyMatchBots),
// exit 0; a rejected file exits 1 with the parser's message on stderr.  Built against the
// library (the defaults are its own) and run by tests/test_exploration.py.
#include <cstdio>

#include "../../katacoffee_amd/csrc/cli_config.h"

static void line(const coffee_exploration_params& e) {
  printf("%d %.9g %.9g %.9g %.9g %.9g\n", (int)e.use_noise_pruning, (double)e.noise_prune_utility_scale,
         (double)e.noise_pruning_cap, (double)e.cpuct_utility_stdev_prior,
         (double)e.cpuct_utility_stdev_prior_weight, (double)e.cpuct_utility_stdev_scale);
}

int main(int argc, char** argv) {
  std::map<std::string, std::string> kv;
  if(argc < 2 || !kccli::readConfig(argv[1], kv))
    return 2;
  kccli::Settings s;
  coffee_match_params_default(&s.sp);  // as the commands do
  coffee_uncertainty_params_default(&s.unc);
  coffee_exploration_params_default(&s.ex);
  const coffee_search_params defSp = s.sp;
  const coffee_uncertainty_params defUnc = s.unc;
  const coffee_exploration_params defEx = s.ex;
  kccli::MatchBot bots[2];
  try {
    kccli::applyConfig(kv, s);
    kccli::applyMatchBots(kv, defSp, defUnc, defEx, bots);
  } catch(const std::invalid_argument& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  line(s.ex);
  line(bots[0].ex);
  line(bots[1].ex);
  return 0;
}
