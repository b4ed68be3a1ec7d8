// Prints what the config layer (cli_config.h, header-only) resolves a config file's root-search
// keys to: one line "wideRootNoise futileVisitsThreshold" for the plain keys (applyConfig, what
// selfplay / gatekeeper / analysis read) and one per bot of `katago match` (applyMatchBots),
// exit 0; a rejected file exits 1 with the parser's message on stderr.  Built against the
// library and run by tests/test_root_search.py.
#include <cstdio>

#include "../../katacoffee_amd/csrc/cli_config.h"

static void line(const coffee_root_search_params& r) {
  printf("%.9g %.9g\n", (double)r.wide_root_noise, (double)r.futile_visits_threshold);
}

int main(int argc, char** argv) {
  std::map<std::string, std::string> kv;
  if(argc < 2 || !kccli::readConfig(argv[1], kv))
    return 2;
  kccli::Settings s;
  coffee_match_params_default(&s.sp);  // as the commands do
  coffee_uncertainty_params_default(&s.unc);
  coffee_exploration_params_default(&s.ex);
  coffee_root_search_params_default(&s.rs);
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
  line(s.rs);
  line(bots[0].rs);
  line(bots[1].rs);
  return 0;
}
