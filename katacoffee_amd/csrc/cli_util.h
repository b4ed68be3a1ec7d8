// Helpers shared by the `katago` subcommands (cli_selfplay.cpp, cli_gatekeeper.cpp):
// the timestamped log, directories, the newest model of a directory, and the SGF line
// of a finished game.  Host-only and header-only, like cli_config.h.
#pragma once
#include <dirent.h>
#include <sys/stat.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <mutex>
#include <sstream>
#include <string>

namespace kccli {

inline std::mutex gLogMu;
inline FILE* gLog = nullptr;
inline void logf(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lk(gLogMu);
  time_t t = time(nullptr);
  char ts[32];
  strftime(ts, sizeof(ts), "%Y-%m-%d %H:%M:%S", localtime(&t));
  fprintf(stdout, "%s: %s\n", ts, buf);
  fflush(stdout);
  if(gLog) {
    fprintf(gLog, "%s: %s\n", ts, buf);
    fflush(gLog);
  }
}

// Newest regular file in dir ("" if none); its mtime in *mt.
inline std::string newestModelOrEmpty(const std::string& dir, time_t* mt) {
  DIR* d = opendir(dir.c_str());
  if(!d)
    return "";
  std::string best;
  time_t bestT = 0;
  while(dirent* e = readdir(d)) {
    if(e->d_name[0] == '.')
      continue;
    std::string p = dir + "/" + e->d_name;
    struct stat st;
    if(stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode) && (best.empty() || st.st_mtime > bestT)) {
      best = p;
      bestT = st.st_mtime;
    }
  }
  closedir(d);
  if(mt)
    *mt = bestT;
  return best;
}

inline std::string modelNameOf(const std::string& path) {
  std::string n = path.substr(path.find_last_of('/') + 1);
  return n.find('.') != std::string::npos ? n.substr(0, n.find('.')) : n;
}

inline void mkdirs(const std::string& path) {
  std::string cur;
  std::stringstream ss(path);
  std::string part;
  if(!path.empty() && path[0] == '/')
    cur = "/";
  while(std::getline(ss, part, '/')) {
    if(part.empty())
      continue;
    cur += part + "/";
    mkdir(cur.c_str(), 0755);
  }
}

// One finished game as an SGF line (sgf.cpp:1526-1700: FF[4] GM[Coffee] SZ WLL PB PW RE,
// moves B[xyd] / W[xyd] with d = a..d for N, W, NW, NE; Coffee draws -- SPEC B16 -- are
// RE[0]).  h: (slot, game number, number of moves, winner); mv [A][2] (cell, direction).
inline std::string sgfGame(int x, int y, int winLen, const std::string& pb, const std::string& pw, const int32_t* h,
                           const uint8_t* mv) {
  const int A = x * y;
  const char* coord = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";
  const char* res = h[3] == 1 ? "B+" : (h[3] == 2 ? "W+" : "0");
  std::string g = "(;FF[4]GM[Coffee]";
  g += x == y ? "SZ[" + std::to_string(x) + "]" : "SZ[" + std::to_string(x) + ":" + std::to_string(y) + "]";
  g += "WLL[" + std::to_string(winLen) + "]PB[" + pb + "]PW[" + pw + "]RE[" + res + "]";
  g += "C[startTurnIdx=0,initTurnNum=0,gameId=" + std::to_string(h[0]) + ":" + std::to_string(h[1]) +
       ",gtype=normal]";
  for(int t = 0; t < h[2] && t < A; t++) {
    const int cell = mv[(size_t)t * 2], d = mv[(size_t)t * 2 + 1];
    g += t % 2 == 0 ? ";B[" : ";W[";
    g += coord[cell % x];
    g += coord[cell / x];
    g += (char)('a' + d);
    g += "]";
    if(t + 1 == h[2])
      g += std::string("C[result=") + res + "]";
  }
  g += ")\n";
  return g;
}

}  // namespace kccli
