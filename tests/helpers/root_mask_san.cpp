// Stand-alone driver of the root restriction rule (rootmask.h) and of the analysis query's
// root keys (cli_analysis_query.h, cli_json.h) for tests/test_analysis_root_cli_parse.py, built
// under AddressSanitizer and UndefinedBehaviorSanitizer.  One request per stdin line:
//   Q <x> <y> <pla> <json>       -> "ok <includePolicy> <mode> <11 words>" | "error <field>|<message>"
//   M <x> <y> <prune> <mode> <n_hist> {<cell> <dir>} <colours: A digits> <legal: W hex words> <avoid: 11 hex words>
//                                -> "mask <W hex words> syms <bits> masked <n> left <n>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <utility>
#include <string>
#include <vector>

#include "cli_analysis_query.h"
#include "rootmask.h"

// SPEC B12: bit 0 flips y, bit 1 flips x, bit 2 transposes (square boards).
static void tables(int X, int Y, std::vector<uint8_t>& cell, std::vector<int8_t>& dir) {
  cell.assign(8 * kc::RM_AREA, 0);
  dir.assign(8 * 5, 0);
  for(int s = 0; s < 8; s++) {
    for(int c = 0; c < X * Y; c++) {
      int x = c % X, y = c / X;
      if(s & 2) x = X - 1 - x;
      if(s & 1) y = Y - 1 - y;
      if((s & 4) && X == Y) std::swap(x, y);
      cell[s * kc::RM_AREA + c] = (uint8_t)(y * X + x);
    }
    const int e = X == Y ? s : (s & 3);
    for(int d = 0; d < 5; d++) {
      int o = d;
      if(d < 4) {
        if(((e & 2) != 0) != ((e & 1) != 0)) o = o == 2 ? 3 : (o == 3 ? 2 : o);
        if(e & 4) o = o == 0 ? 1 : (o == 1 ? 0 : o);
      }
      dir[s * 5 + d] = (int8_t)o;
    }
  }
}

int main() {
  std::string line;
  while(std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    int x = 0, y = 0;
    in >> kind >> x >> y;
    if(kind == "Q") {
      int pla = 0;
      in >> pla;
      std::string json;
      std::getline(in, json);
      kcjson::Object o;
      std::string err, field;
      if(!kcjson::parseLine(json, o, err, &kccli::analysisQuerySchema())) {
        printf("error json|%s\n", err.c_str());
        continue;
      }
      kccli::RootQuery rq;
      if(!kccli::parseRootKeys(o, x, y, pla, rq, err, field)) {
        printf("error %s|%s\n", field.c_str(), err.c_str());
        continue;
      }
      printf("ok %d %d", rq.includePolicy ? 1 : 0, rq.restrict_.mode);
      for(int w = 0; w < COFFEE_ANALYSIS_RESTRICT_WORDS; w++)
        printf(" %x", rq.restrict_.avoid[w]);
      printf("\n");
    } else if(kind == "M") {
      int prune = 0, mode = 0, nh = 0;
      in >> prune >> mode >> nh;
      kc::RootPos p{};
      for(int k = 0; k < 5; k++) {
        p.histCell[k] = -1;
        p.histDir[k] = 4;
      }
      for(int k = 0; k < nh && k < 5; k++)
        in >> p.histCell[k] >> p.histDir[k];
      std::string colours;
      in >> colours;
      const int A = x * y, P = 4 * A, W = (P + 31) / 32;
      for(int c = 0; c < A && c < (int)colours.size(); c++)
        if(colours[c] == '1' || colours[c] == '2')
          p.stones[2 * (colours[c] - '1') + (c >> 6)] |= 1ULL << (c & 63);
      std::vector<uint32_t> legal((size_t)W), mask((size_t)W), avoid(kc::RM_QUERY_WORDS);
      for(auto& w : legal)
        in >> std::hex >> w;
      for(auto& w : avoid)
        in >> std::hex >> w;
      std::vector<uint8_t> sc;
      std::vector<int8_t> sd;
      tables(x, y, sc, sd);
      const kc::RootGeom g{x, y, A, P, sc.data(), sd.data()};
      if(mode != kc::RM_NONE && (P > 32 * kc::RM_QUERY_WORDS || kc::rmBitsPastP(P, avoid.data()))) {
        printf("error avoid|bits past P\n");
        continue;
      }
      uint32_t syms = 0;
      int masked = 0;
      const int left = kc::rmRootMask(g, p, legal.data(), avoid.data(), mode, prune != 0, mask.data(), &syms, &masked);
      printf("mask");
      for(uint32_t w : mask)
        printf(" %x", w);
      printf(" syms %u masked %d left %d\n", syms, masked, left);
    } else {
      printf("error request|unknown\n");
    }
  }
  return 0;
}
