// Prints what the config layer of `katago match` (cli_config.h, header-only) resolves a config
// file to, one line per bot: "name model maxVisits cpuctExploration rootNoiseEnabled use coeff
// exponent maxWeight" (an empty model prints as -), exit 0; a rejected file exits 1 with the
// parser's message on stderr.  Built against the library (the defaults are its own) and run by
// tests/test_match_sides_config.py.
#include <cstdio>
#include <cstring>

#include "../../katacoffee_amd/csrc/cli_config.h"

int main(int argc, char** argv) {
  std::map<std::string, std::string> kv;
  if(argc < 2 || !kccli::readConfig(argv[1], kv))
    return 2;
  coffee_search_params sp;
  coffee_uncertainty_params unc;
  coffee_match_params_default(&sp);  // as the command does
  coffee_uncertainty_params_default(&unc);
  kccli::MatchBot bots[2];
  try {
    kccli::applyMatchBots(kv, sp, unc, bots);
  } catch(const std::invalid_argument& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  for(int i = 0; i < 2; i++)
    printf("%s %s %d %.9g %d %d %.9g %.9g %.9g\n", bots[i].name.c_str(),
           bots[i].model.empty() ? "-" : bots[i].model.c_str(), (int)bots[i].sp.max_visits,
           (double)bots[i].sp.cpuct_exploration, (int)bots[i].sp.root_noise_enabled,
           (int)bots[i].unc.use_uncertainty, (double)bots[i].unc.uncertainty_coeff,
           (double)bots[i].unc.uncertainty_exponent, (double)bots[i].unc.uncertainty_max_weight);
  return 0;
}
