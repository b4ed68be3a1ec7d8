// Prints what the CLI's start-position loader (katacoffee_amd/csrc/cli_startpos.h) makes of
// .sgfs directories and a startposes file, for tests/test_start_positions.py (host only).
//   startpos_load_dump X Y W LOADPROB SEED SGFDIRS|- FILE|-
// One line of counters, then one line per sample: weight, then the moves.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../katacoffee_amd/csrc/cli_startpos.h"

int main(int argc, char** argv) {
  if(argc != 8)
    return 2;
  const std::string dirs = argv[6], file = argv[7];
  const kccli::StartPosLoad ld = kccli::loadStartPositions(dirs == "-" ? "" : dirs, file == "-" ? "" : file, atoi(argv[1]),
                                                           atoi(argv[2]), atoi(argv[3]), atof(argv[4]),
                                                           strtoull(argv[5], nullptr, 10));
  printf("files %lld games %lld candidates %lld duplicates %lld notLoaded %lld wrongGeometry %lld bad %lld kept %zu\n",
         (long long)ld.files, (long long)ld.games, (long long)ld.candidates, (long long)ld.duplicates,
         (long long)ld.notLoaded, (long long)ld.wrongGeometry, (long long)ld.bad, ld.samples.size());
  for(const coffee_start_position& s : ld.samples) {
    printf("%g", (double)s.weight);
    for(int t = 0; t < s.num_moves; t++)
      printf(" %d", (int)s.moves[t]);
    printf("\n");
  }
  return 0;
}
