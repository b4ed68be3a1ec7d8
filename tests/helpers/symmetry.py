"""The board symmetries' cell and direction maps, derived from the oracle's encoder."""
import numpy as np

from oracle import oracle


def symmetry_maps(X, Y, W):
    """symCell[s][c], symDir[s][d] derived from the oracle's (reference-pinned) V1
    encoder, independently of the device tables: a lone own stone at c lights plane 1
    at symCell[s][c]; a last move in direction d lights plane 3 + symDir[s][d]."""
    A = X * Y
    cells = np.zeros((8 * A, A), np.uint8)
    cells[np.arange(8 * A), np.tile(np.arange(A), 8)] = 1
    hc = np.full((8 * A, 5), -1, np.int8)
    hd = np.full((8 * A, 5), 4, np.int8)
    sym = np.repeat(np.arange(8), A).astype(np.int32)
    binp, _ = oracle.encode_batch(X, Y, W, cells, hc, hd, np.ones(8 * A, np.uint8), sym)
    sym_cell = binp[:, 1, :].argmax(axis=1).reshape(8, A)
    cells = np.zeros((32, A), np.uint8)
    cells[:, A // 2] = 2
    hc = np.full((32, 5), -1, np.int8)
    hd = np.full((32, 5), 4, np.int8)
    hc[:, 0] = A // 2
    hd[:, 0] = np.tile(np.arange(4), 8)
    sym = np.repeat(np.arange(8), 4).astype(np.int32)
    binp, _ = oracle.encode_batch(X, Y, W, cells, hc, hd, np.ones(32, np.uint8), sym)
    sym_dir = binp[:, 3:7, :].sum(axis=2).argmax(axis=1).reshape(8, 4)
    return sym_cell, sym_dir


def canonical_source(X, Y, W):
    """src[s][4A]: the canonical-frame policy of a row encoded under symmetry s is the
    symmetric-frame policy gathered at src[s] (direction-major, d A + c)."""
    A = X * Y
    sym_cell, sym_dir = symmetry_maps(X, Y, W)
    src = np.zeros((8, 4 * A), np.int64)
    for s in range(8):
        for d in range(4):
            src[s, d * A:(d + 1) * A] = sym_dir[s, d] * A + sym_cell[s]
    return src
