// Prints the uncertainty settings the commands' config layer (cli_config.h, header-only) reads
// from a config file: "use coeff exponent maxWeight" on stdout, exit 0; a rejected file exits
// 1 with the parser's message on stderr.  Built against the library (the defaults are its own)
// and run by tests/test_uncertainty.py.
#include <cstdio>
#include <cstring>

#include "../../katacoffee_amd/csrc/cli_config.h"

int main(int argc, char** argv) {
  std::map<std::string, std::string> kv;
  if(argc < 2 || !kccli::readConfig(argv[1], kv))
    return 2;
  kccli::Settings s;
  memset(&s.sp, 0, sizeof(s.sp));
  coffee_uncertainty_params_default(&s.unc);  // as the commands do
  try {
    kccli::applyConfig(kv, s);
  } catch(const std::invalid_argument& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  printf("%d %.9g %.9g %.9g\n", (int)s.unc.use_uncertainty, (double)s.unc.uncertainty_coeff,
         (double)s.unc.uncertainty_exponent, (double)s.unc.uncertainty_max_weight);
  return 0;
}
