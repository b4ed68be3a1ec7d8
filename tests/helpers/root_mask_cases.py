"""The root restriction rule restated in numpy from SPEC B12, independently of
the library's symmetry tables, and the positions the root-mask tests share.

Symmetry s: bit 0 flips y, bit 1 flips x, bit 2 transposes (after the flips; square boards
only).  A flip of exactly one axis swaps NW and NE, a transpose swaps N and W."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("coffee_rules", os.path.join(os.path.dirname(__file__), "coffee_rules.py"))
rules = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rules)


def sym_cell(X, Y, s, c):
    x, y = c % X, c // X
    if s & 2:
        x = X - 1 - x
    if s & 1:
        y = Y - 1 - y
    if s & 4:
        x, y = y, x
    return y * X + x


def sym_dir(s, d):
    if bool(s & 1) != bool(s & 2):
        d = {2: 3, 3: 2}.get(d, d)
    if s & 4:
        d = {0: 1, 1: 0}.get(d, d)
    return d


def image(X, Y, s, p):
    A = X * Y
    return sym_dir(s, p // A) * A + sym_cell(X, Y, s, p % A)


def position(X, Y, W, moves):
    """The board after `moves` and what the network's input holds of the history: the last
    five moves, most recent first."""
    b = rules.Board(X, Y, W)
    for m in moves:
        assert not b.finished and b.legal(m % b.A, m // b.A), moves
        b.play(m)
    assert not b.finished, moves
    hist = [(m % b.A, m // b.A) for m in reversed(moves)][:5]
    return b, hist


def features(X, Y, b, hist, s):
    """The input's own features in the frame of symmetry s: stones by colour, the last move's
    cell on its direction's plane, the cells of moves 2-5 ago (everything else in the V1 input
    is derived from these)."""
    A = X * Y
    f = np.zeros((10, A), np.uint8)
    for c in range(A):
        if b.cells[c]:
            f[b.cells[c] - 1, sym_cell(X, Y, s, c)] = 1
    for k, (c, d) in enumerate(hist):
        if k == 0:
            f[2 + sym_dir(s, d), sym_cell(X, Y, s, c)] = 1
        else:
            f[5 + k, sym_cell(X, Y, s, c)] = 1
    return f


def expected(X, Y, W, moves, avoid=None, allow=None, prune=True):
    """The rule: a dict with root (root symmetries), used, legal / mask (bool [P]), orbits (the
    orbits of the legal, not avoided moves under the used symmetries)."""
    A, P = X * Y, 4 * X * Y
    b, hist = position(X, Y, W, moves)
    group = range(8) if X == Y else range(4)
    f0 = features(X, Y, b, hist, 0)
    root = [s for s in group if np.array_equal(features(X, Y, b, hist, s), f0)]
    legal = np.zeros(P, bool)
    legal[b.legal_moves()] = True
    av = np.zeros(P, bool)
    if avoid is not None:
        av[list(avoid)] = True
    if allow is not None:
        av[:] = True
        av[list(allow)] = False
    used = [s for s in root if all(av[image(X, Y, s, p)] for p in np.nonzero(av)[0])]
    mask = av.copy()
    orbits = {}
    for p in np.nonzero(legal & ~av)[0]:
        orb = sorted({image(X, Y, s, int(p)) for s in used})
        orbits[orb[0]] = orb
        if prune and orb[0] < p:
            mask[p] = True
    return {"board": b, "hist": hist, "root": root, "used": used, "legal": legal, "mask": mask, "orbits": orbits,
            "avoid": av}


def library_inputs(b, hist):
    """colours, hist_cell, hist_dir for kc.root_mask."""
    return (np.array(b.cells, np.uint8), np.array([c for c, _ in hist], np.int32),
            np.array([d for _, d in hist], np.int32))


SEED = 5  # chosen so the random openings hold both trivial and nontrivial used groups


def cases():
    """(name, X, Y, W, moves): empty boards, the symmetric one-move positions and seeded random
    legal openings of 1-6 moves."""
    out = [("empty5", 5, 5, 4, []), ("empty7", 7, 7, 5, []), ("empty9", 9, 9, 5, []), ("empty6x4", 6, 4, 3, [])]
    for d in range(4):
        out.append(("centre%d" % d, 5, 5, 4, [d * 25 + 12]))
    out.append(("cornerNW", 5, 5, 4, [2 * 25 + 0]))
    rng = np.random.default_rng(SEED)
    for i in range(24):
        X, Y, W = [(5, 5, 4), (7, 7, 5), (9, 9, 5)][i % 3]
        out.append(("random%d" % i, X, Y, W, rules.random_position(X, Y, W, 1 + i % 6, rng)))
    return out
