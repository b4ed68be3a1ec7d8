// `katago analysis` for Coffee on MI355X: a JSON-lines position analysis service over the
// C ABI's analysis engine (coffee_analysis_*), after the reference's command/analysis.cpp.
//
//   katago analysis -config <cfg> [-model <file>] [-override-config k=v,k=v,...]
//
// One query per line on stdin:
//   {"id":"q1","moves":["ccb","bca"],"maxVisits":50}
// moves are in the SGF writer's three-letter form (sgfGame in cli_util.h): column, row,
// direction a-d, from the empty board, black first.  maxVisits is optional.  One line per
// finished query on stdout, in completion order:
//   {"id":...,"turnNumber":...,"rootInfo":{"visits":...,"winrate":...,"currentPlayer":"B|W"},
//    "moveInfos":[{"move":...,"visits":...,"winrate":...,"prior":...,"lcb":...,"order":...,"pv":[...]},...]}
// moveInfos is sorted by order; winrates and lcb are from the side to move.  A move list that
// ends the game gets "gameOver":true and "winner" ("B", "W" or "0") with no moveInfos.
// A malformed line, an unknown move string, an illegal move or an out-of-range field gets
//   {"id":...,"error":...,"field":...}
// and the service goes on.  End of input finishes the outstanding queries and exits 0.
// Root restrictions (cli_analysis_query.h): the config key rootSymmetryPruning
// (false) and the query keys includePolicy, allowMoves / avoidMoves
// ([{"player":"B","moves":[...],"untilDepth":1}]).  rootInfo carries "symmetries", the used
// ones; with pruning on, a pruned legal move whose orbit's survivor was searched is reported
// as the survivor's entry with move and pv mapped and "isSymmetryOf"; "policy" (when asked)
// has P numbers, -1 at illegal moves.
// Without -model the stand-in network answers.  Config: the search keys of cli_config.h on
// coffee_analysis_params_default, numAnalysisSlots (64), analysisPVLen (15),
// nnCacheSizePowerOfTwo, nnPrecision.
#include <poll.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/katacoffee.h"
#include "cli_analysis_query.h"
#include "cli_config.h"
#include "cli_json.h"
#include "cli_util.h"

using namespace kccli;

namespace {

[[noreturn]] void fail(const std::string& msg) {
  fprintf(stderr, "katago analysis: %s\n", msg.c_str());
  exit(1);
}

void must(int rc, const char* what) {
  if(rc != COFFEE_OK)
    fail(std::string(what) + ": " + coffee_last_error());
}

int parseMove(const std::string& m, int x, int y) { return parseAnalysisMove(m, x, y); }
std::string moveString(int pos, int x, int y) { return analysisMoveString(pos, x, y); }

std::string num(double v) {
  char b[40];
  snprintf(b, sizeof(b), "%.6g", std::isfinite(v) ? v : 0.0);
  return b;
}

void emit(const std::string& line) {
  fputs(line.c_str(), stdout);
  fputc('\n', stdout);
  fflush(stdout);
}

void emitError(const std::string& idJson, const std::string& error, const std::string& field) {
  emit("{\"id\":" + idJson + ",\"error\":" + kcjson::quote(error) + ",\"field\":" + kcjson::quote(field) + "}");
}

// White-perspective win/loss average in [-1, 1] as the winrate of player pla.
double winrateFor(double whiteWL, int pla) {
  const double w = 0.5 * (std::max(-1.0, std::min(1.0, whiteWL)) + 1.0);
  return pla == 2 ? w : 1.0 - w;
}

struct Service {
  int x = 5, y = 5, A = 25, P = 100, maxVisitsCap = 0;
  coffee_analysis* h = nullptr;
  uint64_t nextId = 1;
  std::map<uint64_t, std::string> idJson;  // engine id -> the query's own id, as JSON text
  std::vector<coffee_analysis_query> waiting;  // parsed, not yet accepted by the engine
  std::vector<coffee_analysis_restrict> waitingRestrict;  // beside them
  std::map<uint64_t, RootQuery> rootQuery;  // engine id -> the query's root keys
  bool prune = false;                       // rootSymmetryPruning

  // One input line: an error line at once, or a query queued for the engine.
  void takeLine(const std::string& line) {
    kcjson::Object o;
    std::string err;
    if(!kcjson::parseLine(line, o, err, &analysisQuerySchema())) {
      emitError("null", "malformed query: " + err, "json");
      return;
    }
    std::string id = "null";
    if(const kcjson::Value* v = o.find("id")) {
      if(v->kind == kcjson::Value::STRING)
        id = kcjson::quote(v->s);
      else if(v->kind == kcjson::Value::INT)
        id = std::to_string(v->i);
      else {
        emitError("null", "id must be a string or an integer", "id");
        return;
      }
    } else {
      emitError("null", "missing id", "id");
      return;
    }
    coffee_analysis_query q;
    memset(&q, 0, sizeof(q));
    const kcjson::Value* mv = o.find("moves");
    if(mv && mv->kind != kcjson::Value::STRINGS) {
      emitError(id, "moves must be an array of strings", "moves");
      return;
    }
    const size_t n = mv ? mv->a.size() : 0;
    if(n > (size_t)A) {
      emitError(id, "more moves than the board has cells", "moves");
      return;
    }
    for(size_t t = 0; t < n; t++) {
      const int pos = parseMove(mv->a[t], x, y);
      if(pos < 0) {
        emitError(id, "unknown move '" + mv->a[t] + "' at index " + std::to_string(t), "moves");
        return;
      }
      q.moves[t] = (uint16_t)pos;
    }
    q.num_moves = (int32_t)n;
    if(const kcjson::Value* v = o.find("maxVisits")) {
      if(v->kind != kcjson::Value::INT || v->i < 1 || v->i > maxVisitsCap) {
        emitError(id, "maxVisits must be an integer in 1.." + std::to_string(maxVisitsCap), "maxVisits");
        return;
      }
      q.max_visits = (int32_t)v->i;
    }
    RootQuery rq;
    std::string field;
    if(!parseRootKeys(o, x, y, 1 + (int)(n % 2), rq, err, field)) {
      emitError(id, err, field);
      return;
    }
    q.id = nextId++;
    q.stream = (uint32_t)q.id;
    idJson[q.id] = id;
    rootQuery[q.id] = rq;
    waiting.push_back(q);
    waitingRestrict.push_back(rq.restrict_);
  }

  void submitWaiting() {
    if(waiting.empty())
      return;
    int took = 0;
    must(coffee_analysis_submit2(h, waiting.data(), waitingRestrict.data(), (int)waiting.size(), &took), "submit");
    waiting.erase(waiting.begin(), waiting.begin() + took);
    waitingRestrict.erase(waitingRestrict.begin(), waitingRestrict.begin() + took);
  }

  // One moveInfos entry: child c reported as move `move` with its PV mapped by symmetry sym
  // (0: as searched); survivor >= 0 marks a symmetry copy.
  std::string moveInfo(const coffee_analysis_move& c, int pla, int sym, int survivor) {
    auto img = [&](int pos) { return sym == 0 ? pos : coffee_symmetry_move(x, y, sym, pos); };
    const double wr = winrateFor(c.win_loss_avg, pla);
    // lcb is the mover's utility bound in [-1, 1]; a child without a visit has none
    const double lcb = c.visits > 0 ? 0.5 * ((double)c.lcb + 1.0) : wr;
    std::string o = "{\"move\":\"" + moveString(img(c.move), x, y) + "\",\"visits\":" + std::to_string(c.edge_visits) +
                    ",\"winrate\":" + num(wr) + ",\"prior\":" + num(c.prior) + ",\"lcb\":" + num(lcb) +
                    ",\"order\":" + std::to_string(c.order) + ",\"pv\":[";
    for(int t = 0; t < c.pv_len && t < COFFEE_ANALYSIS_MAX_PV; t++)
      o += std::string(t ? "," : "") + "\"" + moveString(img(c.pv[t]), x, y) + "\"";
    o += "]";
    if(survivor >= 0)
      o += ",\"isSymmetryOf\":\"" + moveString(survivor, x, y) + "\"";
    return o + "}";
  }

  void report(const coffee_analysis_result& r, const coffee_analysis_move* m, const coffee_analysis_root_info& ri,
              const float* policy) {
    const std::string id = idJson[r.id];
    idJson.erase(r.id);
    const RootQuery rq = rootQuery[r.id];
    rootQuery.erase(r.id);
    if(r.status == COFFEE_ANALYSIS_NO_ALLOWED_MOVE) {
      const char* key = rq.restrict_.mode == 2 ? "allowMoves" : "avoidMoves";
      emitError(id, std::string(key) + " leaves no legal move", key);
      return;
    }
    if(r.status == COFFEE_ANALYSIS_ILLEGAL_MOVE) {
      emitError(id, "illegal move at index " + std::to_string(r.info), "moves");
      return;
    }
    std::string o = "{\"id\":" + id + ",\"turnNumber\":" + std::to_string(r.turn);
    const char* cur = r.pla == 1 ? "B" : "W";
    if(r.status != COFFEE_ANALYSIS_OK) {
      const char* w = r.status == COFFEE_ANALYSIS_GAME_OVER && r.info == 1 ? "B" : (r.info == 2 ? "W" : "0");
      o += std::string(",\"rootInfo\":{\"visits\":0,\"winrate\":0.5,\"currentPlayer\":\"") + cur +
           "\"},\"moveInfos\":[],\"gameOver\":true,\"winner\":\"" + w + "\"}";
      emit(o);
      return;
    }
    o += ",\"rootInfo\":{\"visits\":" + std::to_string(r.visits) + ",\"winrate\":" +
         num(winrateFor(r.win_loss_avg, r.pla)) + ",\"currentPlayer\":\"" + cur + "\",\"symmetries\":[";
    bool first = true;
    for(int sy = 0; sy < 8; sy++)
      if((ri.symmetries >> sy) & 1u) {
        o += std::string(first ? "" : ",") + std::to_string(sy);
        first = false;
      }
    o += "]},\"moveInfos\":[";
    const int k = r.num_children;
    std::vector<int> byOrder((size_t)k, 0);
    for(int i = 0; i < k; i++)
      if(m[i].order >= 0 && m[i].order < k)
        byOrder[(size_t)m[i].order] = i;
    for(int r2 = 0; r2 < k; r2++)
      o += std::string(r2 ? "," : "") + moveInfo(m[byOrder[(size_t)r2]], r.pla, 0, -1);
    // symmetry pruning: every pruned legal move whose orbit's survivor was searched is the
    // survivor's entry seen through the lowest used symmetry that takes the survivor to it
    // (the policy marks the legal moves; avoided moves get no copies)
    if(prune && policy && (ri.symmetries & ~1u) != 0) {
      std::vector<int> childOf((size_t)P, -1);
      for(int i = 0; i < k; i++)
        if(m[i].move >= 0 && m[i].move < P)
          childOf[(size_t)m[i].move] = i;
      const bool have = rq.restrict_.mode != 0;
      auto avoided = [&](int p) {
        const bool bit = (rq.restrict_.avoid[p >> 5] >> (p & 31)) & 1u;
        return have && (rq.restrict_.mode == 2 ? !bit : bit);
      };
      for(int r2 = 0; r2 < k; r2++) {
        const coffee_analysis_move& c = m[byOrder[(size_t)r2]];
        std::map<int, int> copies;  // pruned move -> lowest symmetry from the survivor
        for(int sy = 7; sy >= 1; sy--)
          if((ri.symmetries >> sy) & 1u) {
            const int p = coffee_symmetry_move(x, y, sy, c.move);
            if(p > c.move && p < P && policy[p] >= 0.0f && !avoided(p) && childOf[(size_t)p] < 0)
              copies[p] = sy;
          }
        for(const auto& cp : copies)
          o += "," + moveInfo(c, r.pla, cp.second, c.move);
      }
    }
    o += "]";
    if(rq.includePolicy && policy) {
      o += ",\"policy\":[";
      for(int p = 0; p < P; p++)
        o += std::string(p ? "," : "") + (policy[p] < 0.0f ? std::string("-1") : num(policy[p]));
      o += "]";
    }
    emit(o + "}");
  }
};

}  // namespace

int analysisMain(int argc, char** argv) {
  std::string cfgPath, model, overrides;
  for(int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    auto next = [&]() -> std::string {
      if(i + 1 >= argc)
        fail("missing value for " + a);
      return argv[++i];
    };
    if(a == "-config")
      cfgPath = next();
    else if(a == "-model")
      model = next();
    else if(a == "-override-config")
      overrides = next();
    else
      fail("unknown argument " + a);
  }
  if(cfgPath.empty())
    fail("-config is required");
  std::map<std::string, std::string> kv;
  if(!readConfig(cfgPath, kv))
    fail("cannot read config " + cfgPath);
  std::stringstream os(overrides);
  std::string item;
  while(std::getline(os, item, ',')) {
    const size_t eq = item.find('=');
    if(eq != std::string::npos)
      kv[trim(item.substr(0, eq))] = trim(item.substr(eq + 1));
  }
  Settings s;
  coffee_analysis_params_default(&s.sp);
  coffee_uncertainty_params_default(&s.unc);
  coffee_exploration_params_default(&s.ex);
  int slots = 64, pvLen = 15;  // analysis_example.cfg: analysisPVLen 15
  try {
    applyConfig(kv, s);
    applySearchThreadsConfig(ConfigReader{kv, ""}, s.searchThreads, s.virtualLossesPerThread);
    for(auto kd : {std::make_pair("numAnalysisSlots", &slots), std::make_pair("analysisPVLen", &pvLen)}) {
      auto it = kv.find(kd.first);
      if(it == kv.end())
        continue;
      size_t used = 0;
      *kd.second = std::stoi(it->second, &used);
      if(used != it->second.size())
        throw std::invalid_argument(std::string("config key ") + kd.first + ": bad value '" + it->second + "'");
    }
  } catch(const std::invalid_argument& e) {
    fail(e.what());
  } catch(const std::exception&) {
    fail("config: bad value for numAnalysisSlots or analysisPVLen");
  }
  coffee_analysis_config c;
  memset(&c, 0, sizeof(c));
  c.x = s.x;
  c.y = s.y;
  c.win_len = s.winLen;
  c.num_slots = slots;
  c.seed = s.seed ? s.seed : 1;
  c.model_path = model.empty() ? nullptr : model.c_str();
  c.search = s.sp;
  c.nn_cache_log2 = s.nnCacheLog2;
  c.nn_precision = s.nnPrecision;
  c.commit_interval = 8;
  c.query_capacity = 4 * std::max(slots, 1);
  c.max_pv_len = pvLen;
  Service sv;
  must(coffee_analysis_create(&c, &sv.h), "create analysis engine");
  must(coffee_analysis_set_uncertainty(sv.h, &s.unc), "set uncertainty");
  must(coffee_analysis_set_exploration(sv.h, &s.ex), "set exploration");
  must(coffee_analysis_set_root_search(sv.h, &s.rs), "set root search");
  // a round of numAnalysisSlots x threads rows must fit one network launch
  if(coffee_analysis_set_search_threads(sv.h, s.searchThreads, s.virtualLossesPerThread) != COFFEE_OK)
    fail(std::string("config key numSearchThreadsPerAnalysisThread: ") + coffee_last_error());
  // the policy travels with every result: a query's includePolicy prints it, and the symmetry
  // copies read the legal moves off it
  const coffee_analysis_root_options ro{s.rootSymmetryPruning, 1};
  must(coffee_analysis_set_root_options(sv.h, &ro), "set root options");
  sv.prune = s.rootSymmetryPruning != 0;
  sv.x = s.x;
  sv.y = s.y;
  sv.A = s.x * s.y;
  sv.P = 4 * sv.A;
  sv.maxVisitsCap = s.sp.max_visits;  // the node pools are sized for the config's visits
  fprintf(stderr, "katago analysis: %dx%d win %d, %d slots, %d visits, %s\n", s.x, s.y, s.winLen, slots,
          s.sp.max_visits, model.empty() ? "stand-in network" : model.c_str());
  if(s.searchThreads > 1)
    fprintf(stderr, "katago analysis: %d search threads per slot, %g virtual losses per thread\n", s.searchThreads,
            (double)s.virtualLossesPerThread);
  std::vector<coffee_analysis_result> hdr((size_t)c.query_capacity);
  std::vector<coffee_analysis_move> mv((size_t)c.query_capacity * sv.P);
  std::vector<coffee_analysis_root_info> rinfo((size_t)c.query_capacity);
  std::vector<float> pol((size_t)c.query_capacity * sv.P);
  std::string buf;
  bool eof = false, skipping = false;  // skipping: inside an over-long line already reported
  char chunk[65536];
  while(!eof || !sv.idJson.empty() || !sv.waiting.empty()) {
    const bool busy = !sv.idJson.empty();
    if(!eof) {
      // wait for input only while nothing is being searched
      pollfd pf{0, POLLIN, 0};
      const int pr = poll(&pf, 1, busy ? 0 : -1);
      if(pr > 0) {
        const ssize_t got = read(0, chunk, sizeof(chunk));
        if(got <= 0)
          eof = true;
        else
          buf.append(chunk, (size_t)got);
      }
      size_t nl;
      while((nl = buf.find('\n')) != std::string::npos) {
        const std::string line = buf.substr(0, nl);
        buf.erase(0, nl + 1);
        if(skipping)
          skipping = false;
        else if(line.find_first_not_of(" \t\r") != std::string::npos)
          sv.takeLine(line);
      }
      if(buf.size() > kcjson::MAX_LINE) {
        // an over-long line: reported once, its rest skipped up to the next newline
        if(!skipping)
          sv.takeLine(buf);
        skipping = true;
        buf.clear();
      }
      if(eof && !skipping && buf.find_first_not_of(" \t\r") != std::string::npos) {
        sv.takeLine(buf);  // a last line without a newline
        buf.clear();
      }
    }
    sv.submitWaiting();
    if(sv.idJson.empty())
      continue;
    must(coffee_analysis_step(sv.h, 16, nullptr), "step");
    int n = 0;
    must(coffee_analysis_drain2(sv.h, c.query_capacity, hdr.data(), mv.data(), rinfo.data(), pol.data(), &n), "drain");
    for(int i = 0; i < n; i++)
      sv.report(hdr[(size_t)i], mv.data() + (size_t)i * sv.P, rinfo[(size_t)i], pol.data() + (size_t)i * sv.P);
  }
  coffee_analysis_stats st;
  must(coffee_analysis_stats_get(sv.h, &st), "stats");
  fprintf(stderr, "katago analysis: %llu queries, %llu rounds, %llu playouts\n",
          (unsigned long long)st.queries_finished, (unsigned long long)st.rounds, (unsigned long long)st.playouts);
  must(coffee_analysis_destroy(sv.h), "destroy");
  return 0;
}
