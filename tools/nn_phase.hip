// Phase timing of the fused network kernel (shader-clock stamps of thread 0 of the first
// workgroups).  Build: make -C tools nn_phase ; run on the GPU box:
// tools/_build/nn_phase [boards] [path (engine.h NNPath): 5 fast (default), 1 accurate,
// 3 corrected, 4 accurate-nb2] [indirect: 1 = launch with a device-side count and a row
// index (reversed rows), the way the self-play engine does]
// Stamps (nn.hip NN_PHASE): 0 entry, 1 input unpacked, 2 stem conv, 3 + 4b .. 6 + 4b the
// marks of block b, 40 last conv2, 41 head conv; of the last gpool block 49 its mid's
// start, 50 g-epilogue + barrier, 51 pool, 52 gpool linear, 55 r-epilogue + barrier; of the
// heads 53 stage epilogue + barrier, 56 head weights staged, 54 pool + barrier, 57 / 58 the
// policy-gpool / value linear (58 after the barrier), 42 value outputs, 59 policy stores
// (thread 0's end of the kernel).
#define KC_NN_PROFILE
#include "../katacoffee_amd/csrc/nn.hip"

#include <cstdio>
#include <random>

using namespace kc;

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 4096;  // <= 5 x CUs: the small-batch (5-board) instance
  ModelHost m = randomModel(modelCfgByName("b6c96"), 1);
  const int path = argc > 2 ? atoi(argv[2]) : NN_FAST;
  NNEngine eng(m, 5, 5, 4, path);
  const int words = (15 * 25 + 63) / 64;
  std::vector<uint64_t> in((size_t)n * words);
  std::mt19937_64 rng(1);
  for(auto& w : in)
    w = rng() & rng();
  uint64_t* din;
  float* dout;
  KC_HIP(hipMalloc(&din, in.size() * 8));
  KC_HIP(hipMalloc(&dout, (size_t)n * 104 * 4));
  KC_HIP(hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice));
  const bool indirect = argc > 3 && atoi(argv[3]) != 0;
  int *dcount = nullptr, *drow = nullptr;
  if(indirect) {
    std::vector<int> rows(n);
    for(int i = 0; i < n; i++)
      rows[i] = n - 1 - i;
    KC_HIP(hipMalloc(&dcount, 4));
    KC_HIP(hipMalloc(&drow, (size_t)n * 4));
    KC_HIP(hipMemcpy(dcount, &n, 4, hipMemcpyHostToDevice));
    KC_HIP(hipMemcpy(drow, rows.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  for(int it = 0; it < 3; it++)
    eng.forward(n, din, dout, nullptr, dcount, drow);
  KC_HIP(hipDeviceSynchronize());
  unsigned long long ph[4][64];
  KC_HIP(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_nnPhase), sizeof(ph)));
  const char* names[64] = {};
  names[0] = "start";
  names[1] = "input unpacked";
  names[2] = "stem conv";
  for(int b = 0; b < 6; b++) {
    static char buf[6][4][48];
    snprintf(buf[b][0], 48, "blk%d start (prev conv)", b);
    snprintf(buf[b][1], 48, "blk%d bn1", b);
    snprintf(buf[b][2], 48, "blk%d conv1", b);
    snprintf(buf[b][3], 48, "blk%d mid (bn2/gpool)", b);
    names[3 + 4 * b] = buf[b][0];
    names[4 + 4 * b] = buf[b][1];
    names[5 + 4 * b] = buf[b][2];
    names[6 + 4 * b] = buf[b][3];
  }
  names[40] = "last conv2";
  names[41] = "tip + head conv";
  names[53] = "head stage epilogue";
  names[56] = "head weights staged";
  names[54] = "head pool";
  names[57] = "policy-gpool linear";
  names[58] = "value linear";
  names[42] = "value outputs";
  names[59] = "policy tail (end)";
  int order[] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18,
                 19, 20, 21, 22, 23, 24, 25, 26, 40, 41, 53, 56, 54, 57, 58, 42, 59};
  auto d = [&](int wg, int a, int b) { return (long long)(ph[wg][a] - ph[wg][b]); };
  long long tot[4] = {};
  for(int wg = 0; wg < 2; wg++) {
    printf("workgroup %d (cycles since previous mark)\n", wg);
    unsigned long long prev = ph[wg][0];
    for(int i : order) {
      // phase k+1 of block b is stamped before the next; skip unset slots
      if(ph[wg][i] == 0)
        continue;
      printf("  %-24s %8lld\n", names[i] ? names[i] : "?", (long long)(ph[wg][i] - prev));
      prev = ph[wg][i];
    }
    tot[wg] = (long long)(prev - ph[wg][0]);
    printf("  gpool mid (last gpool block): g-epilogue %lld  pool %lld  gpool linear %lld  r-epilogue %lld  = %lld\n",
           d(wg, 50, 49), d(wg, 51, 50), d(wg, 52, 51), d(wg, 55, 52), d(wg, 55, 49));
    printf("  heads after the head conv: %lld ; non-conv head+input: unpack %lld\n", d(wg, 59, 41), d(wg, 1, 0));
    printf("  total %lld cycles\n", tot[wg]);
    printf("  wall to stamp 42 %.1f us (s_memrealtime) -> tick %.3f GHz\n", (ph[wg][63] - ph[wg][62]) / 100.0,
           (double)(ph[wg][42] - ph[wg][0]) / ((ph[wg][63] - ph[wg][62]) * 10.0));
  }
  printf("SUMMARY boards %d path %d indirect %d total_wg0 %lld total_wg1 %lld unpack %lld gpool_mid %lld heads %lld\n", n,
         path, (int)indirect, tot[0], tot[1], d(0, 1, 0), d(0, 55, 49), d(0, 59, 41));
  return 0;
}
