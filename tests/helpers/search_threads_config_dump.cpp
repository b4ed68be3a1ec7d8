// Prints what the config layer (cli_config.h, header-only) resolves a config file's parallel-
// playout keys to: a first line "threads virtualLossesPerThread" as `katago analysis` reads them
// (applyConfig, then applySearchThreadsConfig) and a second as the other commands do (applyConfig
// alone: the keys are ignored), exit 0; a file either rejects exits 1 with the parser's message
// on stderr.  Built against the
// library (the defaults are its own) and run by tests/test_search_threads.py.
#include <cstdio>

#include "../../katacoffee_amd/csrc/cli_config.h"

int main(int argc, char** argv) {
  std::map<std::string, std::string> kv;
  if(argc < 2 || !kccli::readConfig(argv[1], kv))
    return 2;
  kccli::Settings s;
  coffee_analysis_params_default(&s.sp);  // as the command does
  coffee_uncertainty_params_default(&s.unc);
  coffee_exploration_params_default(&s.ex);
  kccli::Settings other = s;
  try {
    kccli::applyConfig(kv, other);
  } catch(const std::invalid_argument& e) {
    fprintf(stderr, "other commands: %s\n", e.what());
    return 1;
  }
  try {
    kccli::applyConfig(kv, s);
    kccli::applySearchThreadsConfig(kccli::ConfigReader{kv, ""}, s.searchThreads, s.virtualLossesPerThread);
  } catch(const std::invalid_argument& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  printf("%d %.9g\n", s.searchThreads, (double)s.virtualLossesPerThread);
  printf("%d %.9g\n", other.searchThreads, (double)other.virtualLossesPerThread);
  return 0;
}
