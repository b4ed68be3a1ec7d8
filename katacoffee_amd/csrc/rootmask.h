// Root move restrictions of an analysis query (reference rootSymmetryPruning
// setup.cpp:639-644, allowMoves / avoidMoves analysis.cpp:1030-1097): the set of root moves the
// search treats as unavailable -- the query's avoid set and, with pruning on, every move that
// has a symmetric image at a lower policy position.  Integer code over plain arrays, the same
// on host and device: the device hands each lane a strided share of the cells and positions
// and combines the shares with ballots, the host runs the share (0, 1).
#pragma once
#include <stdint.h>

#ifndef KC_HD
#define KC_HD inline  // a host-only translation unit without the HIP headers
#endif

namespace kc {

constexpr int RM_AREA = 100;   // row length of the symmetry tables (MAX_AREA)
constexpr int RM_WORDS = 13;   // ceil(MAX_P / 32)
constexpr int RM_QUERY_WORDS = 11;  // words of a query's avoid set (coffee_analysis_restrict)
enum { RM_NONE = 0, RM_AVOID = 1, RM_ALLOW = 2 };

// The geometry's symmetry tables (DTables::symCell / symDir, SPEC B12).
struct RootGeom {
  int X, Y, A, P;
  const uint8_t* symCell;  // [8][RM_AREA]
  const int8_t* symDir;    // [8][5]
};
// The position as the network's input sees it: stones (black lo, hi, white lo, hi: bit c of
// the 128-bit set is cell c), the last five moves (cell -1: none; most recent first).
struct RootPos {
  uint64_t stones[4];
  int histCell[5], histDir[5];
};

KC_HD int rmColour(const RootPos& r, int c) {
  const int w = c >> 6, b = c & 63;
  return (int)((r.stones[w] >> b) & 1ULL) + 2 * (int)((r.stones[2 + w] >> b) & 1ULL);
}
KC_HD bool rmBit(const uint32_t* bits, int p) { return (bits[p >> 5] >> (p & 31)) & 1u; }
// The image of policy position dir * A + cell under symmetry s.
KC_HD int rmImage(const RootGeom& g, int s, int p) {
  const int d = p / g.A, c = p - d * g.A;
  return (int)g.symDir[s * 5 + d] * g.A + (int)g.symCell[s * RM_AREA + c];
}
// Every symmetry the geometry has: all eight on a square board, the four without a transpose
// otherwise (tables.cpp folds the transposing ones onto those).
KC_HD uint32_t rmGeomSyms(const RootGeom& g) { return g.X == g.Y ? 0xFFu : 0x0Fu; }

// The symmetries of `cand` under which the packed V1 input differs from the identity's, as far
// as the history decides it: the last move keeps its cell and its direction (its plane is the
// symmetric direction's), the moves two to five ago keep their cells.
KC_HD uint32_t rmHistoryBroken(const RootGeom& g, const RootPos& r, uint32_t cand) {
  uint32_t broken = 0;
  for(int s = 1; s < 8; s++) {
    if(!((cand >> s) & 1u))
      continue;
    bool ok = true;
    const int h0 = r.histCell[0], d0 = r.histDir[0];
    if(h0 >= 0 && d0 >= 0 && d0 < 4)
      ok = (int)g.symCell[s * RM_AREA + h0] == h0 && (int)g.symDir[s * 5 + d0] == d0;
    for(int k = 1; k < 5; k++) {
      const int h = r.histCell[k];
      if(h >= 0 && (int)g.symCell[s * RM_AREA + h] != h)
        ok = false;
    }
    if(!ok)
      broken |= 1u << s;
  }
  return broken;
}
// ... and as far as the stones of the cells c0, c0 + stride, ... decide it.  (Everything else
// in the input -- the legal plane, the run planes -- follows from the stones, the last move
// and the geometry, which the symmetries of rmGeomSyms preserve.)
KC_HD uint32_t rmStonesBroken(const RootGeom& g, const RootPos& r, uint32_t cand, int c0, int stride) {
  uint32_t broken = 0;
  for(int c = c0; c < g.A; c += stride) {
    const int col = rmColour(r, c);
    for(int s = 1; s < 8; s++)
      if(((cand >> s) & 1u) && rmColour(r, (int)g.symCell[s * RM_AREA + c]) != col)
        broken |= 1u << s;
  }
  return broken;
}
// The symmetries of `cand` that move an avoided position among p0, p0 + stride, ... out of the
// avoid set.  (A symmetry permutes the positions, so one that maps the set into itself maps it
// onto itself.)
KC_HD uint32_t rmAvoidBroken(const RootGeom& g, const uint32_t* avoid, uint32_t cand, int p0, int stride) {
  uint32_t broken = 0;
  for(int p = p0; p < g.P; p += stride) {
    if(!rmBit(avoid, p))
      continue;
    for(int s = 1; s < 8; s++)
      if(((cand >> s) & 1u) && !rmBit(avoid, rmImage(g, s, p)))
        broken |= 1u << s;
  }
  return broken;
}
// Whether position p is masked: avoided, or legal and with an image under a used symmetry at a
// lower position (the survivor of an orbit is its lowest position).  avoid: nullptr for none.
KC_HD bool rmMasked(const RootGeom& g, const uint32_t* avoid, uint32_t used, bool prune, int p, bool legal) {
  if(avoid && rmBit(avoid, p))
    return true;
  if(!prune || !legal)
    return false;
  for(int s = 1; s < 8; s++)
    if(((used >> s) & 1u) && rmImage(g, s, p) < p)
      return true;
  return false;
}

// A query's avoid set over the P positions from its RM_QUERY_WORDS words: the words themselves
// (mode avoid) or their complement within P (mode allow).  out: ceil(P / 32) words, bits >= P 0.
KC_HD void rmAvoidWords(int P, const uint32_t* query, int mode, uint32_t* out) {
  const int W = (P + 31) / 32;
  for(int w = 0; w < W; w++) {
    uint32_t x = w < RM_QUERY_WORDS ? query[w] : 0u;
    if(mode == RM_ALLOW)
      x = ~x;
    const int left = P - 32 * w;
    if(left < 32)
      x &= (1u << left) - 1u;
    out[w] = x;
  }
}
// Whether a query's words name a position >= P.
KC_HD bool rmBitsPastP(int P, const uint32_t* query) {
  for(int w = 0; w < RM_QUERY_WORDS; w++) {
    const int left = P - 32 * w;
    const uint32_t valid = left >= 32 ? ~0u : (left <= 0 ? 0u : (1u << left) - 1u);
    if(query[w] & ~valid)
      return true;
  }
  return false;
}

// The whole rule, serially (the host entry point; the device runs the same functions over
// lane shares in analysisRefill).  legal: P bits.  query / mode: the avoid or allow words
// (mode RM_NONE: ignored).  mask: ceil(P / 32) words out.  Returns the number of legal moves
// left unmasked; *symsOut the used symmetries, *maskedOut the masked legal moves.
KC_HD int rmRootMask(const RootGeom& g, const RootPos& r, const uint32_t* legal, const uint32_t* query, int mode,
                     bool prune, uint32_t* mask, uint32_t* symsOut, int* maskedOut) {
  uint32_t used = rmGeomSyms(g);
  used &= ~rmHistoryBroken(g, r, used);
  used &= ~rmStonesBroken(g, r, used, 0, 1);
  uint32_t avoid[RM_WORDS];
  const bool have = mode != RM_NONE;
  if(have) {
    rmAvoidWords(g.P, query, mode, avoid);
    used &= ~rmAvoidBroken(g, avoid, used, 0, 1);
  }
  const int W = (g.P + 31) / 32;
  for(int w = 0; w < W; w++)
    mask[w] = 0;
  int left = 0, masked = 0;
  for(int p = 0; p < g.P; p++) {
    const bool lg = rmBit(legal, p);
    const bool m = rmMasked(g, have ? avoid : nullptr, used, prune, p, lg);
    if(m)
      mask[p >> 5] |= 1u << (p & 31);
    if(lg) {
      left += m ? 0 : 1;
      masked += m ? 1 : 0;
    }
  }
  *symsOut = used;
  *maskedOut = masked;
  return left;
}

}  // namespace kc
