"""The Coffee rules in plain Python, for tests that need legal move lists and the boards they
lead to without a device (Board::isLegal board.cpp:185-227, the win test and the
no-legal-move draw as kc_board.h states them).

A move is a policy position dir * A + cell; cell = y * X + x; directions 0 N, 1 W, 2 NW, 3 NE
name the axis through the cell (both ways)."""
import numpy as np

DIRS = [(0, -1), (-1, 0), (-1, -1), (1, -1)]
OK, ILLEGAL_MOVE, GAME_OVER, NO_LEGAL_MOVE = 0, 1, 2, 3


class Board:
    def __init__(self, X, Y, W):
        self.X, self.Y, self.W, self.A = X, Y, W, X * Y
        self.cells = [0] * (X * Y)  # 0 empty, 1 black, 2 white
        self.pla = 1
        self.last_cell, self.last_dir = -1, 4
        self.turn = 0
        self.finished, self.winner = False, 0

    def line(self, cell, d):
        """Cells on the axis d through cell, without the cell itself."""
        x0, y0 = cell % self.X, cell // self.X
        out = []
        for s in (-1, 1):
            x, y = x0 + s * DIRS[d][0], y0 + s * DIRS[d][1]
            while 0 <= x < self.X and 0 <= y < self.Y:
                out.append(y * self.X + x)
                x, y = x + s * DIRS[d][0], y + s * DIRS[d][1]
        return out

    def legal(self, cell, d):
        if self.cells[cell] != 0:
            return False
        if self.last_cell >= 0 and self.last_dir < 4 and cell not in self.line(self.last_cell, self.last_dir):
            return False
        return any(self.cells[c] == 0 for c in self.line(cell, d))

    def legal_moves(self):
        return [d * self.A + c for d in range(4) for c in range(self.A) if self.legal(c, d)]

    def run(self, cell, d):
        col = self.cells[cell]
        x0, y0 = cell % self.X, cell // self.X
        n = 1
        for s in (-1, 1):
            x, y = x0 + s * DIRS[d][0], y0 + s * DIRS[d][1]
            while 0 <= x < self.X and 0 <= y < self.Y and self.cells[y * self.X + x] == col:
                n += 1
                x, y = x + s * DIRS[d][0], y + s * DIRS[d][1]
        return n

    def play(self, move):
        cell, d = move % self.A, move // self.A
        mover = self.pla
        self.cells[cell] = mover
        self.last_cell, self.last_dir = cell, d
        self.turn += 1
        self.pla = 3 - mover
        if max(self.run(cell, k) for k in range(4)) >= self.W:
            self.finished, self.winner = True, mover
        elif not self.legal_moves():
            self.finished, self.winner = True, 0


def replay(X, Y, W, moves):
    """(status, info, board) of a move list from the empty board, as the device's check of a
    start position reports it: the first move that is out of range, illegal or follows the
    game's end is ILLEGAL_MOVE with its index; a list that ends the game is GAME_OVER with the
    winner, or NO_LEGAL_MOVE for the draw of a player without a move."""
    b = Board(X, Y, W)
    for t, m in enumerate(moves):
        if b.finished or m >= 4 * b.A or not b.legal(m % b.A, m // b.A):
            return ILLEGAL_MOVE, t, b
        b.play(m)
    if b.finished:
        if b.winner == 0 and b.turn < b.A:
            return NO_LEGAL_MOVE, 0, b
        return GAME_OVER, b.winner, b
    return OK, 0, b


def random_position(X, Y, W, length, rng):
    """A legal move list of `length` moves that does not end the game (rng: numpy Generator)."""
    while True:
        b = Board(X, Y, W)
        moves = []
        while len(moves) < length and not b.finished:
            lm = b.legal_moves()
            m = int(lm[rng.integers(len(lm))])
            b.play(m)
            moves.append(m)
        if not b.finished:
            return moves


def random_finished_game(X, Y, W, rng, max_len):
    """A legal move list that ends the game with a winner within max_len moves."""
    while True:
        b = Board(X, Y, W)
        moves = []
        while not b.finished and len(moves) < max_len:
            lm = b.legal_moves()
            m = int(lm[rng.integers(len(lm))])
            b.play(m)
            moves.append(m)
        if b.finished and b.winner != 0:
            return moves


def planes012(board):
    """Planes 0-2 of the V1 encoding of the board for the player to move: [3][A] uint8
    (on board, own stones, opponent's stones)."""
    c = np.array(board.cells)
    return np.stack([np.ones(board.A, np.uint8), (c == board.pla).astype(np.uint8),
                     (c == 3 - board.pla).astype(np.uint8)])
