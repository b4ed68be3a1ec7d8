"""Per-side match settings and the shared net on the device (coffee_match_create2).

The yardstick for "each side searches with its own parameters" is the analysis engine, which
the oracle pins: a search of the match engine is stepped in lockstep with an analysis engine
created with that side's parameters and uncertainty setting, on the same position, stream,
game number and counter, and trees, root priors and game state are compared bit for bit every
round (as tests/test_gpu_start_positions.py does for a search from a start position).

Everything is 5x5/4 with the stand-in network, NN cache off, node_cap 128 and commit interval 1
unless stated."""
import glob
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("coffee_rules", os.path.join(REPO, "tests", "helpers",
                                                                            "coffee_rules.py"))
cr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cr)

SEED, CAP = 11, 128
INFO_KEYS = ("phase", "rootK", "liveCount", "turn", "pla", "lastCell", "lastDir", "rngCtr")
# side 0: few visits, root noise, two root symmetries, uncertainty weighting
SIDE0 = dict(max_visits=12, cpuct_exploration=1.1, root_noise_enabled=1, root_num_symmetries_to_sample=2,
             use_uncertainty=1)
# side 1: more visits, a narrow search, no noise, the most visited move without LCB or temperature
SIDE1 = dict(max_visits=20, cpuct_exploration=0.6, root_fpu_reduction_max=0.1, root_noise_enabled=0,
             use_lcb_for_selection=0, chosen_move_temperature=0.0, chosen_move_temperature_early=0.0)


@pytest.fixture(scope="module")
def b2c32(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("sides") / "b2c32.cfnn")
    kc.write_random_model("b2c32", 0xBEEF, p)
    return p


def _base():
    return kc.default_match_params(max_visits=16, init_games_with_policy=0)


def _side_params(spec):
    """(SearchParams, UncertaintyParams) of a side given as field overrides on _base()."""
    sp, un = _base(), kc.default_uncertainty_params()
    for k, v in spec.items():
        setattr(sp if hasattr(sp, k) else un, k, v)
    return sp, un


def candidate_colour(slot, game_num):
    return 1 if (slot + game_num) % 2 == 0 else 2


def _side_of(slot, info):
    return 1 if info["pla"] == candidate_colour(slot, info["gameNum"]) else 0


def _state(e, slots, cap=CAP):
    out = []
    for s in slots:
        n, ed = e.game_tree(s, cap)
        out.append((e.game_info(s), n.copy(), ed.copy(), e.root_policy(s).copy()))
    return out


def _assert_same_state(a, b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], (what, s, x[0], y[0])
        for u, v in zip(x[1:], y[1:]):
            np.testing.assert_array_equal(u, v, err_msg="%s slot %d" % (what, s))


def _run(e, checkpoints, G):
    """Steps to each checkpoint; returns the states there and every record, in (slot, game) order."""
    states, heads, moves, done = [], [], [], 0
    for c in checkpoints:
        while done < c:
            n = min(100, c - done)
            e.step(n)
            done += n
            h, m = e.drain_games()
            heads.append(h.copy())
            moves.append(m.copy())
        states.append(_state(e, range(G)))
    h, m = np.concatenate(heads), np.concatenate(moves)
    order = np.lexsort((h[:, 1], h[:, 0]))
    return states, h[order], m[order]


# ---------------------------------------------------------------------------------------
# 1. Equal sides change nothing.

@pytest.mark.parametrize("variant", ["standin_ci1", "b2c32_cache_ci16_stagger"])
def test_equal_sides_change_nothing(b2c32, variant):
    G, p = 8, _base()
    kw = dict(num_games=G, seed=SEED, node_cap=CAP, commit_interval=1, search=p)
    if variant != "standin_ci1":
        kw.update(candidate_path=b2c32, nn_cache_log2=10, commit_interval=16, start_stagger=16,
                  nn_precision="accurate")
    runs = []
    for sides in (None, ((p, None), (p, None))):
        e = kc.Match(5, 5, 4, sides=sides, **kw)
        runs.append(_run(e, [1, 30, 97, 300], G))
        st = e.stats()
        assert st["errors"] == 0 and st["games_dropped"] == 0
        e.close()
    (sa, ha, ma), (sb, hb, mb) = runs
    for c, x, y in zip([1, 30, 97, 300], sa, sb):
        _assert_same_state(x, y, "round %d" % c)
    np.testing.assert_array_equal(ha, hb)
    np.testing.assert_array_equal(ma, mb)


# ---------------------------------------------------------------------------------------
# 2 / 3 / 4c. Each side searches with its own parameters.

class Lockstep:
    """A per-side match engine and, per (slot, side), an analysis engine with that side's
    parameters; follow() steps one search of a slot in lockstep with its analysis twin."""

    def __init__(self, X, Y, W, G, model=None, share_net=False, swap=False):
        self.X, self.Y, self.W, self.A, self.G = X, Y, W, X * Y, G
        self.model = model
        self.specs = [_side_params(SIDE0), _side_params(SIDE1)]
        kw = dict(baseline_path=model, candidate_path=model, nn_precision="accurate") if model else {}
        self.m = kc.Match(X, Y, W, num_games=G, seed=SEED, node_cap=CAP, commit_interval=1, search=_base(),
                          sides=(SIDE0, SIDE1), share_net=share_net, **kw)
        self.swap = swap  # control: the analysis twins get the other side's parameters
        self.ans = {}
        self.moves = [[] for _ in range(G)]
        self.seen = [0] * G
        self.game = [0] * G
        self.sides_seen = [[] for _ in range(G)]

    def _twin(self, s, side):
        if (s, side) not in self.ans:
            sp, un = self.specs[side ^ 1 if self.swap else side]
            kw = dict(model_path=self.model, nn_precision="accurate") if self.model else {}
            an = kc.Analysis(self.X, self.Y, self.W, num_slots=1, seed=SEED, node_cap=CAP, query_capacity=4,
                             search=sp, **kw)
            an.set_uncertainty(un)
            self.ans[(s, side)] = (an, sp.max_visits)
        return self.ans[(s, side)]

    def start(self, s):
        """Submits slot s's search that is about to start to its twin; returns (twin, side, limit)."""
        gi = self.m.game_info(s)
        assert gi["phase"] == 0 and gi["rootK"] == 0, gi  # a root evaluation that has not begun
        assert gi["gameNum"] == self.game[s] and gi["turn"] == len(self.moves[s])
        side = _side_of(s, gi)
        an, limit = self._twin(s, side)
        assert an.submit([dict(id=1000 * s + gi["turn"] + 1, moves=self.moves[s], max_visits=limit, stream=s,
                               game_num=gi["gameNum"], rng_counter=gi["rngCtr"])]) == 1
        self.sides_seen[s].append(side)
        return an, side, limit

    def after_round(self, s, an, side, limit, r, diffs):
        """Compares slot s with its twin after a round both have run.  Returns True when the
        search was committed in this round.  diffs: None asserts, a list collects."""
        def check(ok, what):
            if diffs is None:
                assert ok, (s, r, what)
            elif not ok:
                diffs.append((s, r, what))
        gi = self.m.game_info(s)
        if gi["moves"] > self.seen[s]:
            # the commit: the twin reports in the same round, so both reached the side's visit limit together
            h, mv = an.drain()
            check(len(h) == 1, "the twin finishes in the round of the commit")
            if len(h) == 1:
                check(int(h[0]["status"]) == 0 and int(h[0]["visits"]) == limit, "root visits at the commit")
            self.seen[s] = gi["moves"]
            if gi["gameNum"] == self.game[s]:
                played = gi["lastDir"] * self.A + gi["lastCell"]
                assert gi["turn"] == len(self.moves[s]) + 1 and gi["lastCell"] >= 0
                self.moves[s].append(played)
                if side == 1 and len(h) == 1 and not self.swap:
                    kids = mv[0][:int(h[0]["num_children"])]
                    best = [int(k["move"]) for k in kids if int(k["order"]) == 0]
                    check(best == [played], "side 1 plays the analysis result's best move")
            else:
                self.game[s], self.moves[s] = gi["gameNum"], []
            return True
        ai = an.game_info(0)
        for k in INFO_KEYS:
            check(gi[k] == ai[k], k)
        for u, v in zip(self.m.game_tree(s, CAP), an.game_tree(0, CAP)):
            check(np.array_equal(u, v), "tree")
        if gi["phase"] == 1:
            check(np.array_equal(self.m.root_policy(s), an.root_policy(0)), "root policy")
        return False

    def follow_all(self, searches, diffs=None, max_rounds=400):
        """The next `searches` searches of every slot, all slots in lockstep with their twins."""
        cur = {s: self.start(s) for s in range(self.G)}
        left = {s: searches for s in range(self.G)}
        for r in range(max_rounds):
            if not cur:
                return
            self.m.step(1)
            for s in sorted(cur):
                an, side, limit = cur[s]
                an.step(1)
                if self.after_round(s, an, side, limit, r, diffs):
                    left[s] -= 1
                    if left[s] > 0 and diffs is None:
                        cur[s] = self.start(s)
                    else:
                        del cur[s]
                elif diffs and any(d[0] == s for d in diffs):
                    del cur[s]  # control: the slot's first difference is enough
        assert not cur, "searches did not finish"

    def skip_to_game(self, s, game, max_rounds=3000):
        """Steps until slot s stands at the first search of game number `game` (no comparison)."""
        for _ in range(max_rounds):
            gi = self.m.game_info(s)
            if gi["gameNum"] == game:
                assert gi["phase"] == 0 and gi["rootK"] == 0 and gi["turn"] == 0, gi
                self.game[s], self.moves[s], self.seen[s] = game, [], gi["moves"]
                return
            self.m.step(1)
        raise AssertionError("game %d did not start" % game)

    def follow_one(self, s, max_rounds=100):
        an, side, limit = self.start(s)
        for r in range(max_rounds):
            self.m.step(1)
            an.step(1)
            if self.after_round(s, an, side, limit, r, None):
                return side
        raise AssertionError("the search did not finish")

    def close(self):
        assert self.m.stats()["errors"] == 0
        for an, _ in self.ans.values():
            an.close()
        self.m.close()


def _control(X, Y, W, G, **kw):
    """The twins with the two parameter sets swapped: every slot must differ within its first search."""
    c = Lockstep(X, Y, W, G, swap=True, **kw)
    diffs = []
    c.follow_all(1, diffs=diffs)
    c.close()
    assert {d[0] for d in diffs} == set(range(G)), diffs


def test_each_side_searches_with_its_own_parameters_5x5():
    G = 4
    ls = Lockstep(5, 5, 4, G)
    ls.follow_all(6)
    for s in range(G):
        # the sides alternate move by move, the first mover of game 0 by the colour rule
        first = 1 if candidate_colour(s, 0) == 1 else 0
        assert ls.sides_seen[s] == [first ^ (t & 1) for t in range(6)], (s, ls.sides_seen[s])
    assert {ls.sides_seen[s][0] for s in range(G)} == {0, 1}  # both colour pairings occur
    # slot 0's next game: the colours, and with them the sides, have swapped
    ls.skip_to_game(0, 1)
    side = ls.follow_one(0)
    assert side == 1 - ls.sides_seen[0][0]
    ls.close()
    _control(5, 5, 4, G)


def test_each_side_searches_with_its_own_parameters_7x7():
    ls = Lockstep(7, 7, 5, 2)  # NI = 4
    ls.follow_all(3)
    assert {ls.sides_seen[s][0] for s in range(2)} == {0, 1}
    ls.close()
    _control(7, 7, 5, 2)


def test_per_side_parameters_with_a_shared_net(b2c32):
    ls = Lockstep(5, 5, 4, 4, model=b2c32, share_net=True)
    ls.follow_all(3)
    st = ls.m.stats()
    assert st["nn_evals"][1] == 0 and st["nn_evals"][0] > 0
    ls.close()


# ---------------------------------------------------------------------------------------
# 4. Shared net.

def _shared(b2c32, share, cache=0, ci=1, G=8):
    return kc.Match(5, 5, 4, num_games=G, baseline_path=b2c32, candidate_path=b2c32, seed=SEED, node_cap=CAP,
                    commit_interval=ci, nn_cache_log2=cache, nn_precision="accurate", search=_base(),
                    share_net=share)


def test_shared_net_equals_two_instances_cache_off(b2c32):
    G, runs, stats = 8, [], []
    for share in (True, False):
        e = _shared(b2c32, share)
        runs.append(_run(e, [1, 30, 200], G))
        stats.append(e.stats())
        e.close()
    (sa, ha, ma), (sb, hb, mb) = runs
    for c, x, y in zip([1, 30, 200], sa, sb):
        _assert_same_state(x, y, "round %d" % c)
    np.testing.assert_array_equal(ha, hb)
    np.testing.assert_array_equal(ma, mb)
    shared, two = stats
    assert sum(shared["nn_evals"]) == sum(two["nn_evals"]) > 0
    assert shared["nn_evals"][1] == 0 and shared["nn_batch_peak"][1] == 0 and shared["nn_precision"][1] == 0
    assert two["nn_evals"][1] > 0 and two["nn_batch_peak"][1] > 0
    assert shared["errors"] == 0 and two["errors"] == 0


def test_shared_net_with_cache_is_reproducible_and_legal(b2c32):
    G, runs = 8, []
    for _ in range(2):
        e = _shared(b2c32, True, cache=10, ci=16)
        runs.append(_run(e, [600], G))
        st = e.stats()
        assert st["errors"] == 0 and st["games_dropped"] == 0 and st["nn_evals"][1] == 0
        e.close()
    (sa, ha, ma), (sb, hb, mb) = runs
    _assert_same_state(sa[0], sb[0], "round 600")
    np.testing.assert_array_equal(ha, hb)
    np.testing.assert_array_equal(ma, mb)
    assert len(ha) >= G // 2
    for h, m in zip(ha, ma):
        moves = [int(m[t, 1]) * 25 + int(m[t, 0]) for t in range(h[2])]
        status, info, board = cr.replay(5, 5, 4, moves)
        if h[3] != 0:
            assert status == cr.GAME_OVER and info == h[3], (h, status, info)
        else:  # a draw: the board is full, or the player to move has no move
            assert status in (cr.GAME_OVER, cr.NO_LEGAL_MOVE) and board.winner == 0, (h, status, info)
        assert h[4] == candidate_colour(h[0], h[1])


def test_shared_cache_carries_the_error_for_the_side_that_weights_by_it(b2c32):
    """Shared net, cache on, side 0 with uncertainty weighting and side 1 without: an entry that
    side 1's search wrote must still carry the net's short-term error, or side 0's hit on it
    weights the leaf as if the error were 0 -- exactly max_weight, which no evaluation gets
    (the error is a softplus, > 0, so the weight coeff / (err + coeff / max_weight) stays below it).
    Word 21 of every expanded node of a side-0 tree is checked after every round; side 1's
    trees export 0 there."""
    G = 8
    un = kc.default_uncertainty_params()
    m = kc.Match(5, 5, 4, num_games=G, baseline_path=b2c32, candidate_path=b2c32, seed=SEED, node_cap=CAP,
                 commit_interval=1, nn_cache_log2=10, nn_precision="accurate", search=_base(),
                 sides=(dict(max_visits=16, use_uncertainty=1), dict(max_visits=16)), share_net=True)
    checked = {0: 0, 1: 0}
    for r in range(160):
        m.step(1)
        for s in range(G):
            gi = m.game_info(s)
            if gi["phase"] != 1:
                continue
            side = _side_of(s, gi)
            nodes, _ = m.game_tree(s, CAP)
            expanded = nodes[((nodes[:, 10] >> 24) & 1) == 1]
            w = expanded[:, 21].copy().view(np.float32)
            checked[side] += len(w)
            if side == 0:
                assert np.all((w > 0) & (w < un.uncertainty_max_weight)), (r, s, w)
            else:
                assert np.all(expanded[:, 21] == 0), (r, s)
    st = m.stats()
    m.close()
    assert st["errors"] == 0 and st["nn_evals"][1] == 0
    assert checked[0] > 1000 and checked[1] > 1000, checked
    # the cache was in use: fewer network rows than playouts plus root evaluations could explain
    assert st["nn_evals"][0] < st["playouts"], st


# ---------------------------------------------------------------------------------------
# 5. Self-play is untouched in the same process.

def test_selfplay_unaffected_by_a_per_side_match_in_the_process(b2c32):
    kw = dict(num_games=16, max_visits=16, seed=5, node_cap=64, commit_interval=4, nn_cache_log2=8)

    def rows(with_match):
        sp = kc.Selfplay(5, 5, 4, **kw)
        sp.step(300)
        if with_match:
            m = kc.Match(5, 5, 4, num_games=8, baseline_path=b2c32, candidate_path=b2c32, seed=SEED, node_cap=CAP,
                         commit_interval=2, nn_cache_log2=8, nn_precision="accurate", search=_base(),
                         sides=(SIDE0, SIDE1), share_net=True)
            m.step(300)
            st = m.stats()
            assert st["games_dropped"] == 0 and st["errors"] == 0 and st["moves"] > 0
            m.close()
        sp.step(300)
        assert sp.stats()["rows_dropped"] == 0
        r = sp.drain_rows()
        sp.close()
        # games that finish in one commit launch take their row places in any order
        order = np.lexsort((r["meta"][:, 2], r["meta"][:, 1], r["meta"][:, 0]))
        return {k: v[order] for k, v in r.items()}

    a, b = rows(False), rows(True)
    assert len(a["meta"]) > 0
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_set_uncertainty_is_refused_with_per_side_settings():
    m = kc.Match(5, 5, 4, num_games=2, node_cap=CAP, search=_base(), sides=(SIDE0, SIDE1))
    with pytest.raises(kc.CoffeeError, match="sides"):
        m.set_uncertainty(use_uncertainty=1)
    m.close()


# ---------------------------------------------------------------------------------------
# 6. `katago match`.

def _katago_match(tmp_path, name, model):
    out = tmp_path / name
    cmd = [os.path.join(REPO, "katacoffee_amd", "katago"), "match", "-config",
           os.path.join(REPO, "configs", "match_coffee5.cfg"), "-sgf-output-dir", str(out), "-log-file",
           str(tmp_path / (name + ".log")), "-override-config",
           "nnModelFile=%s,maxVisits0=4,maxVisits1=16,numGamesTotal=8,numGameThreads=4,seed=77,"
           "botName0=quick,botName1=deep,nnCacheSizePowerOfTwo=10,nnPrecision=accurate" % model]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return r, out


def test_katago_match_cli(tmp_path, b2c32):
    r, out = _katago_match(tmp_path, "a", b2c32)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log
    assert "the net is shared" in log
    files = glob.glob(str(out / "*.sgfs"))
    assert len(files) == 1
    games = open(files[0]).read().splitlines()
    assert len(games) == 8
    tally = {"w": 0, "d": 0, "l": 0}
    seen = set()
    for g in games:
        pb, pw = re.search(r"PB\[(\w+)\]", g).group(1), re.search(r"PW\[(\w+)\]", g).group(1)
        slot, num = map(int, re.search(r"gameId=(\d+):(\d+)", g).groups())
        res = re.search(r"RE\[([^\]]+)\]", g).group(1)
        assert num * 4 + slot < 8
        seen.add((slot, num))
        # bot 1 ("deep") is black in game n of slot s iff s + n is even
        assert (pb, pw) == (("deep", "quick") if (slot + num) % 2 == 0 else ("quick", "deep")), g
        deep_black = pb == "deep"
        if res == "0":
            tally["d"] += 1
        elif (res == "B+") == deep_black:
            tally["w"] += 1
        else:
            tally["l"] += 1
    assert seen == {(s, n) for s in range(4) for n in range(2)}
    final = re.findall(r"after (\d+) games: W-D-L (\d+)-(\d+)-(\d+) \(as black (\d+)-(\d+)-(\d+), as white "
                       r"(\d+)-(\d+)-(\d+)\), score ([0-9.]+), Elo (\S+) \[(\S+), (\S+)\], LOS ([0-9.]+)%", log)
    assert final, log
    f = final[-1]
    n, w, d, lo = (int(x) for x in f[:4])
    assert n == 8 and w + d + lo == 8 and (w, d, lo) == (tally["w"], tally["d"], tally["l"])
    assert [int(f[4 + k]) + int(f[7 + k]) for k in range(3)] == [w, d, lo]
    assert float(f[10]) == pytest.approx(kc.match_elo(w, d, lo)["score"], abs=1e-4)
    # the same seed writes the same file
    r2, out2 = _katago_match(tmp_path, "b", b2c32)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    files2 = glob.glob(str(out2 / "*.sgfs"))
    assert [os.path.basename(x) for x in files2] == [os.path.basename(files[0])]
    assert open(files2[0]).read() == open(files[0]).read()
