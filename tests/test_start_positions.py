"""Start positions without a device: the table's 64-bit thresholds against a float64
restatement, the pick (the kernels' own code run on the host) against its stated rule and a
Python restatement of the game stream, and the CLI's loaders of .sgfs and startposes files."""
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------
# 1. Thresholds.

def _tables():
    rng = np.random.default_rng(0)
    one = [([1, 2, 3], 2.5)]
    three = [([1, 2], 1.0), ([4], 0.0), ([], 3.0)]
    seventy = [(list(range(int(rng.integers(0, 20)))), float(rng.integers(0, 5)) + 0.25 * (i % 3 == 0))
               for i in range(70)]
    return {"n1": one, "three": three, "seventy": seventy}


@pytest.mark.parametrize("lam", [0.0, 0.5, -0.5])
@pytest.mark.parametrize("name", ["n1", "three", "seventy"])
def test_thresholds_match_float64(name, lam):
    table = _tables()[name]
    cum = kc.start_positions_thresholds(table, lam)
    w = np.array([t[1] for t in table], np.float64)
    turns = np.array([len(t[0]) for t in table], np.float64)
    p = w * np.exp(-turns * lam)
    p = p / p.sum()
    c = [int(x) for x in cum]
    assert all(a <= b for a, b in zip(c, c[1:])) and c[-1] == M64
    diffs = np.array([(b - a) / 2.0 ** 64 for a, b in zip([0] + c, c)])
    np.testing.assert_allclose(diffs, p, rtol=0, atol=1e-12)
    for i, (_, wi) in enumerate(table):
        if wi == 0.0:
            assert c[i] == (c[i - 1] if i else 0)


def test_thresholds_errors():
    good = [([1], 1.0), ([2], 1.0)]
    for bad in ([([1], -1.0), ([2], 1.0)], [([1], float("nan"))], [([1], float("inf"))], [([1], 0.0), ([], 0.0)], []):
        with pytest.raises(kc.CoffeeError):
            kc.start_positions_thresholds(bad, 0.0)
    with pytest.raises(kc.CoffeeError):
        kc.start_positions_thresholds(good, 11.0)
    assert len(kc.start_positions_thresholds(good, 0.0)) == 2


# ---------------------------------------------------------------------------------------
# 2. Pick.

def _first_below(cum, r):
    for i, c in enumerate(cum):
        if r < c:
            return i
    return next(i for i, c in enumerate(cum) if c == M64)  # r = 2^64 - 1: the last positive sample


def test_index_is_the_first_threshold_above_the_draw():
    arrays = [[M64], [5, 5, 9, M64], [0, 0, 1 << 63, M64, M64], [1 << 62, 1 << 63, 3 << 62, M64],
              [7, M64, M64, M64]]
    for cum in arrays:
        rs = {0, 1, M64, M64 - 1, 1 << 63}
        for c in cum:
            rs |= {c, max(c - 1, 0), min(c + 1, M64)}
        for r in sorted(rs):
            assert kc.start_position_index(cum, r) == _first_below(cum, r), (cum, r)
    big = sorted(int(x) for x in np.random.default_rng(1).integers(0, 1 << 63, 100000, dtype=np.uint64))
    big[-1] = M64
    for r in (0, big[0], big[49999], big[49999] - 1, big[-2], M64):
        assert kc.start_position_index(big, r) == _first_below(big, r)


def _mix64(z):
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _python_pick(seed, slot, game, prob, cum):
    """startGame's draws restated: stream seed, two hash draws, u = uni(), r = next()."""
    s = _mix64(seed ^ _mix64((slot << 32) | game))
    nxt = lambda ctr: _mix64(s ^ ((ctr * 0xd1342543de82ef95) & M64))
    u = np.float32(nxt(3) >> 40) * np.float32(1.0 / 16777216.0)
    if not u < np.float32(prob):
        return -1, 3
    return _first_below(cum, nxt(4)), 4


def test_pick_follows_the_game_stream():
    table = [([1], 1.0), ([2, 3], 0.0), ([], 2.0), ([4, 5, 6], 1.5)]
    cum = [int(c) for c in kc.start_positions_thresholds(table, 0.25)]
    seen = set()
    for slot in range(40):
        for game in range(5):
            got = kc.start_position_pick(99, slot, game, 0.6, cum, with_counter=True)
            assert got == _python_pick(99, slot, game, 0.6, cum), (slot, game)
            seen.add(got[0])
    assert seen == {-1, 0, 2, 3}


def test_zero_weight_entry_is_never_picked():
    table = [([1], 1.0), ([2], 0.0), ([3], 1.0), ([4], 0.0)]
    cum = kc.start_positions_thresholds(table, 0.0)
    counts = np.zeros(5, np.int64)
    for slot in range(1000):
        for game in range(100):
            counts[kc.start_position_pick(7, slot, game, 1.0, cum)] += 1
    assert counts[1] == 0 and counts[3] == 0 and counts[4] == 0  # [4]: index -1, never with prob 1
    assert counts[0] + counts[2] == 100000 and abs(int(counts[0]) - 50000) < 1000  # 6 sigma of a fair coin


def test_off_makes_no_draw():
    cum = kc.start_positions_thresholds([([1], 1.0)], 0.0)
    for slot in range(50):
        assert kc.start_position_pick(3, slot, 0, 0.0, cum, with_counter=True) == (-1, 2)
        assert kc.start_position_pick(3, slot, 0, 0.5, None, with_counter=True) == (-1, 2)
        assert kc.start_position_pick(3, slot, 0, 1.0, cum, with_counter=True) == (0, 4)


# ---------------------------------------------------------------------------------------
# 3. CLI loaders.

@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sp") / "startpos_load_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe,
                    os.path.join(REPO, "tests", "helpers", "startpos_load_dump.cpp")], check=True)

    def run(x, y, w, load_prob, seed, dirs, file):
        out = subprocess.run([exe, str(x), str(y), str(w), str(load_prob), str(seed), dirs or "-", file or "-"],
                             check=True, capture_output=True, text=True).stdout.splitlines()
        f = out[0].split()
        counters = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
        samples = [(float(l.split()[0]), [int(t) for t in l.split()[1:]]) for l in out[1:]]
        return counters, samples

    return run


def _sgf(x, y, w, moves, a=None):
    a = a or x * y
    coord = "abcdefghijklmnopqrstuvwxyz"
    s = "(;FF[4]GM[Coffee]SZ[%d]WLL[%d]PB[m]PW[m]RE[B+]C[startTurnIdx=0,initTurnNum=0,gameId=0:0,gtype=normal]" % (x, w)
    for t, m in enumerate(moves):
        cell, d = m % a, m // a
        s += ";%s[%s%s%s]" % ("BW"[t % 2], coord[cell % x], coord[cell // x], "abcd"[d])
    return s + "C[result=B+])\n"


def test_cli_loaders(dump, tmp_path):
    g1 = [0, 25 + 6, 50 + 12, 75 + 18, 3]          # five moves: prefixes of length 1..4
    g2 = [0, 25 + 6, 7, 8]                         # shares its first two prefixes with g1
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir()
    d2.mkdir()
    (d1 / "0001.sgfs").write_text(_sgf(5, 5, 4, g1) + _sgf(5, 5, 4, g2))
    (d2 / "0002.sgfs").write_text(_sgf(7, 7, 5, [0, 1, 2], a=49) + _sgf(5, 5, 5, g1))  # other geometries
    (d2 / "notes.txt").write_text("not a game file\n")
    pos = tmp_path / "x.startposes.txt"
    pos.write_text('{"moves":["aaa","bbb"],"weight":2.5}\n'          # a duplicate of g1's second prefix
                   '{"moves":["cca","dab"],"weight":0.5}\n'
                   '{"moves":[],"weight":1.0}\n'
                   '{"moves":["aaa"],"weight":1.0,"xSize":7,"ySize":7,"winLen":5}\n'
                   '{"board":"....","nextPla":"B"}\n'
                   '{"moves":["zza"]}\n')
    c, s = dump(5, 5, 4, 1.0, 1, "%s, %s" % (d1, d2), str(pos))
    want = [(1.0, g1[:n]) for n in (1, 2, 3, 4)] + [(1.0, g2[:3])] + [(0.5, [12, 25 + 3]), (1.0, [])]
    assert s == want
    assert c == dict(files=3, games=4, candidates=4 + 3 + 3, duplicates=3, notLoaded=0, wrongGeometry=3, bad=2, kept=7)
    # startPosesLoadProb: the kept set is a subset in order, the same for the same seed
    c1, s1 = dump(5, 5, 4, 0.5, 42, "%s,%s" % (d1, d2), str(pos))
    c2, s2 = dump(5, 5, 4, 0.5, 42, "%s,%s" % (d1, d2), str(pos))
    assert (c1, s1) == (c2, s2) and c1["kept"] + c1["notLoaded"] == 7
    it = iter(want)
    assert all(x in it for x in s1)
    kept = {tuple(map(tuple, [m for _, m in dump(5, 5, 4, 0.5, seed, str(d1), "")[1]])) for seed in range(8)}
    assert len(kept) > 1  # other seeds keep other sets
    assert dump(5, 5, 4, 0.0, 1, str(d1), str(pos))[0]["kept"] == 0
