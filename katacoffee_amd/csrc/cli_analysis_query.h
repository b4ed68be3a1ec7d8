// The root-restriction keys of a `katago analysis` query line (the reference's
// analysis.cpp:1030-1097): includePolicy, and allowMoves / avoidMoves as lists of
// {"player": "B" | "W", "moves": [...], "untilDepth": 1}.  Host-only and header-only, over
// cli_json.h and the C ABI's structs; compiles without the library.
#pragma once
#include <cstring>
#include <string>

#include "../../include/katacoffee.h"
#include "cli_json.h"

namespace kccli {

static const char* const ANALYSIS_COORD = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";

// "ccb" -> policy position dir * A + cell, or -1.
inline int parseAnalysisMove(const std::string& m, int x, int y) {
  if(m.size() != 3)
    return -1;
  const char* cx = strchr(ANALYSIS_COORD, m[0]);
  const char* cy = strchr(ANALYSIS_COORD, m[1]);
  if(!m[0] || !m[1] || !cx || !cy || cx - ANALYSIS_COORD >= x || cy - ANALYSIS_COORD >= y || m[2] < 'a' || m[2] > 'd')
    return -1;
  return (m[2] - 'a') * x * y + (int)(cy - ANALYSIS_COORD) * x + (int)(cx - ANALYSIS_COORD);
}

inline std::string analysisMoveString(int pos, int x, int y) {
  const int A = x * y, cell = pos % A;
  std::string s;
  s += ANALYSIS_COORD[cell % x];
  s += ANALYSIS_COORD[cell / x];
  s += (char)('a' + pos / A);
  return s;
}

// The schema of a query line for kcjson::parseLine.
inline const kcjson::Schema& analysisQuerySchema() {
  static const char* const bools[] = {"includePolicy", nullptr};
  static const char* const lists[] = {"allowMoves", "avoidMoves", nullptr};
  static const kcjson::Schema s{bools, lists};
  return s;
}

struct RootQuery {
  coffee_analysis_restrict restrict_;  // mode 0: the query's root is not restricted
  bool includePolicy = false;
  RootQuery() { memset(&restrict_, 0, sizeof(restrict_)); }
};

// Reads includePolicy, allowMoves and avoidMoves of a parsed line for a position with player
// `pla` (1 black, 2 white) to move on an x * y board.  False with the message and the field's
// name for: a wrong type, both lists, an allowMoves list without exactly one entry, an entry
// without player / moves / untilDepth, an unknown player or move, untilDepth other than 1
// (only the root is restricted), and a board whose positions do not fit the set.  Entries for
// the player who is not to move have no effect.
inline bool parseRootKeys(const kcjson::Object& o, int x, int y, int pla, RootQuery& out, std::string& error,
                          std::string& field) {
  auto bad = [&](const char* f, const std::string& msg) {
    field = f;
    error = msg;
    return false;
  };
  out = RootQuery();
  if(const kcjson::Value* v = o.find("includePolicy")) {
    if(v->kind != kcjson::Value::BOOL)
      return bad("includePolicy", "includePolicy must be true or false");
    out.includePolicy = v->i != 0;
  }
  const kcjson::Value* allow = o.find("allowMoves");
  const kcjson::Value* avoid = o.find("avoidMoves");
  if(allow && avoid)
    return bad("allowMoves", "allowMoves and avoidMoves cannot both be given");
  if(!allow && !avoid)
    return true;
  const char* key = allow ? "allowMoves" : "avoidMoves";
  const kcjson::Value* list = allow ? allow : avoid;
  if(list->kind != kcjson::Value::OBJECTS)
    return bad(key, std::string(key) + " must be an array of {\"player\",\"moves\",\"untilDepth\"} objects");
  if(allow && list->objs.size() != 1)
    return bad(key, "allowMoves must have exactly one entry");
  const int P = 4 * x * y;
  if(P > 32 * COFFEE_ANALYSIS_RESTRICT_WORDS)
    return bad(key, std::string(key) + " needs a board of at most " + std::to_string(32 * COFFEE_ANALYSIS_RESTRICT_WORDS) +
                        " policy positions");
  bool any = false;
  for(const kcjson::Object& e : list->objs) {
    const kcjson::Value* pl = e.find("player");
    const kcjson::Value* mv = e.find("moves");
    const kcjson::Value* ud = e.find("untilDepth");
    if(!pl || pl->kind != kcjson::Value::STRING)
      return bad(key, std::string(key) + ": player must be \"B\" or \"W\"");
    int who = 0;
    if(pl->s == "B" || pl->s == "b")
      who = 1;
    else if(pl->s == "W" || pl->s == "w")
      who = 2;
    else
      return bad(key, std::string(key) + ": player must be \"B\" or \"W\"");
    if(!mv || mv->kind != kcjson::Value::STRINGS)
      return bad(key, std::string(key) + ": moves must be an array of strings");
    if(!ud || ud->kind != kcjson::Value::INT)
      return bad("untilDepth", std::string(key) + ": untilDepth must be an integer");
    if(ud->i != 1)
      return bad("untilDepth", std::string(key) + ": untilDepth must be 1 (only the root is restricted)");
    for(const std::string& m : mv->a) {
      const int pos = parseAnalysisMove(m, x, y);
      if(pos < 0)
        return bad(key, std::string(key) + ": unknown move '" + m + "'");
      if(who == pla)
        out.restrict_.avoid[pos >> 5] |= 1u << (pos & 31);
    }
    any = any || who == pla;
  }
  if(any)
    out.restrict_.mode = allow ? 2 : 1;
  return true;
}

}  // namespace kccli
