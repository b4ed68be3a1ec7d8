"""Two-network match play on the device (kc.Match) against the CPU oracle.

The oracle plays one network, but with cheap searches off it clears the tree before every
search, and its set_net callback runs after the round's selection, when info(slot) shows
the root player and the game number.  A games=1 oracle of global slot s whose callback
applies the colour rule and hands the (single) row to net 0 or net 1 therefore plays
exactly the match game of that slot: game state, canonical trees and root priors are
compared bit for bit.  Net 0 is the stand-in network, net 1 a seeded random b2c32 on the
accurate kernels; the oracle is fed the same device forwards (kc.fake_net,
kc.Network.forward), whose rows do not depend on the batch they are evaluated in.
"""
import numpy as np
import pytest

import katacoffee_amd as kc
from oracle import oracle

pytestmark = pytest.mark.gpu

INFO_KEYS = [("phase", "phase"), ("rootK", "rootK"), ("liveCount", "nodeCount"), ("gameNum", "gameNum"),
             ("turn", "turn"), ("pla", "pla"), ("playouts", "playouts"), ("nnEvals", "nnEvals"),
             ("moves", "movesMade"), ("gamesFinished", "gamesFinished"), ("rngCtr", "rngCtr"),
             ("lastCell", "lastCell"), ("lastDir", "lastDir")]
SEED = 11
CHECKPOINTS = [1, 30, 97, 700, 1500]


def _compare_game(gpu, ora, g, og, done):
    gi, oi = gpu.game_info(g), ora.info(og)
    for a, b in INFO_KEYS:
        assert gi[a] == oi[b], (done, g, a, gi[a], oi[b])
    gn, ge = gpu.game_tree(g)
    on, oe = ora.game_tree(og)
    np.testing.assert_array_equal(gn, on, err_msg="round %d game %d nodes" % (done, g))
    np.testing.assert_array_equal(ge, oe, err_msg="round %d game %d edges" % (done, g))
    if gi["phase"] == 1:
        np.testing.assert_array_equal(gpu.root_policy(g), ora.root_noised(og))


def candidate_colour(slot, game_num):
    """The colour rule: the candidate is black (1) in game n of global slot s iff s + n is even."""
    return 1 if (slot + game_num) % 2 == 0 else 2


@pytest.fixture(scope="module")
def b2c32(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("match") / "b2c32.cfnn")
    kc.write_random_model("b2c32", 0xBEEF, p)
    return p


class Routed:
    """A games=1 oracle of global slot `slot` whose evaluations are routed by the colour rule
    to forwards[0] (baseline) or forwards[1] (candidate).  rows[n]: rows net n evaluated;
    moves_of[game number]: the moves seen through info, when polled after every round."""

    def __init__(self, X, Y, W, slot, visits, forwards, ci=1, stagger=0, **play):
        self.slot = slot
        self.ora = oracle.Selfplay(X, Y, W, games=1, max_visits=visits, node_cap=128, seed=SEED, slot_base=slot,
                                   commit_interval=ci, start_stagger=stagger, **play)
        self.rows = [0, 0]
        self.largest = 0
        self.moves_of = {}
        self._seen = 0

        def route(packed):
            i = self.ora.info(0)
            net = 1 if i["pla"] == candidate_colour(slot, i["gameNum"]) else 0
            self.rows[net] += len(packed)
            self.largest = max(self.largest, len(packed))
            return forwards[net](packed)

        self.ora.set_net(route)

    def rounds_polled(self, n):
        """n rounds one by one, appending every move that appears in info.  A game's last
        move cannot be read this way: the commit that plays it starts the slot's next game
        in the same round, whose info shows no last move."""
        for _ in range(n):
            self.ora.rounds(1)
            i = self.ora.info(0)
            if i["movesMade"] > self._seen:
                assert i["movesMade"] == self._seen + 1
                self._seen = i["movesMade"]
                if i["lastCell"] >= 0:
                    self.moves_of.setdefault(i["gameNum"], []).append((i["lastCell"], i["lastDir"]))
                else:
                    self.moves_of.setdefault(i["gameNum"] - 1, []).append(None)  # the finished game's last move


def _forwards(X, Y, W, model_path):
    net = kc.Network(model_path, X, Y, W, precision="accurate")
    return net, [lambda p: kc.fake_net(X, Y, W, p), net.forward]


def _match(X, Y, W, G, visits, model_path, ci=1, stagger=0, cache=0, cap=None, **play):
    # the oracle's search parameters are coffee_search_params_default's
    return kc.Match(X, Y, W, num_games=G, candidate_path=model_path, seed=SEED, node_cap=128, commit_interval=ci,
                    start_stagger=stagger, nn_cache_log2=cache, nn_batch_cap=G if cap is None else cap,
                    nn_precision="accurate", search=kc.default_search_params(max_visits=visits), **play)


def _replay(X, Y, W, header, moves):
    """Replays every record move by move on the device rules (kc.rules_batch / kc.play_batch):
    each move legal when played; returns (finished, winner, has_legal after the last move)."""
    n, A = len(header), X * Y
    cells = np.zeros((n, A), np.uint8)
    lc, ld = np.full(n, -1, np.int8), np.full(n, 4, np.int8)
    pla = np.ones(n, np.uint8)
    fin, win = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for t in range(int(header[:, 2].max())):
        on = np.nonzero(header[:, 2] > t)[0]
        assert np.all(fin[on] == 0), "a record goes on after its game ended"
        mv = moves[on, t, 1].astype(np.int32) * A + moves[on, t, 0].astype(np.int32)
        assert np.all(moves[on, t, 0] < A) and np.all(moves[on, t, 1] < 4)
        legal, _ = kc.rules_batch(X, Y, W, cells[on], lc[on], ld[on], pla[on])
        assert np.all(legal[np.arange(len(on)), mv] == 1), "illegal move at turn %d" % t
        oc, f, w, _, _, _ = kc.play_batch(X, Y, W, cells[on], lc[on], ld[on], pla[on], mv)
        cells[on], fin[on], win[on] = oc, f, w
        lc[on], ld[on] = moves[on, t, 0].astype(np.int8), moves[on, t, 1].astype(np.int8)
        pla[on] = 3 - pla[on]
    _, has = kc.rules_batch(X, Y, W, cells, lc, ld, pla)
    return fin, win, has


def _assert_records_replay(X, Y, W, header, moves):
    fin, win, has = _replay(X, Y, W, header, moves)
    for i in range(len(header)):
        if header[i, 3] != 0:
            assert fin[i] == 1 and win[i] == header[i, 3], (i, header[i], fin[i], win[i])
        else:  # a draw: the board is full, or nobody can move
            assert win[i] == 0 and (fin[i] == 1 or has[i] == 0), (i, header[i])
        assert header[i, 4] == candidate_colour(header[i, 0], header[i, 1]), header[i]


# ---------------------------------------------------------------------------------------
# 1. Routed parity, composed.

@pytest.fixture(scope="module")
def ci1_run(b2c32):
    """The commit-interval-1 run of tests 1 and 2: the device engine and one routed oracle
    per sampled slot, the oracles polled after every round for their move lists.  Mismatches
    at the checkpoints are kept for test 1 to report."""
    X, Y, W, G, visits = 5, 5, 4, 64, 24
    slots = [0, 1, 2, 33, 63]
    net, fw = _forwards(X, Y, W, b2c32)
    gpu = _match(X, Y, W, G, visits, b2c32)
    oras = [Routed(X, Y, W, s, visits, fw) for s in slots]
    failures, recs, done = [], [], 0
    for chunk in CHECKPOINTS:
        for at in range(done, chunk, 400):  # the record buffer holds 2 G games: drain twice a game length
            gpu.step(min(400, chunk - at))
            recs.append(gpu.drain_games())
        for r in oras:
            r.rounds_polled(chunk - done)
        done = chunk
        for r in oras:
            try:
                _compare_game(gpu, r.ora, r.slot, 0, done)
            except AssertionError as e:
                failures.append(e)
    out = dict(X=X, Y=Y, W=W, slots=slots, oras=oras, failures=failures, stats=gpu.stats(),
               records=(np.concatenate([h for h, _ in recs]), np.concatenate([m for _, m in recs])))
    gpu.close()
    net.close()
    return out


def test_routed_parity_ci1(ci1_run):
    assert not ci1_run["failures"], ci1_run["failures"][0]
    for r in ci1_run["oras"]:
        i = r.ora.info(0)
        assert i["gamesFinished"] >= 2, (r.slot, i)  # both colourings occurred in every sampled slot
        assert r.largest <= 1 and min(r.rows) > 0, (r.slot, r.rows, r.largest)
    assert ci1_run["stats"]["errors"] == 0 and ci1_run["stats"]["games_dropped"] == 0


def test_routed_parity_ci16_stagger(b2c32):
    X, Y, W, G, visits = 5, 5, 4, 64, 24
    net, fw = _forwards(X, Y, W, b2c32)
    gpu = _match(X, Y, W, G, visits, b2c32, ci=16, stagger=29)
    oras = [Routed(X, Y, W, s, visits, fw, ci=16, stagger=29) for s in [0, 1, 2, 33, 63]]
    done = 0
    for chunk in CHECKPOINTS:
        gpu.step(chunk - done)
        for r in oras:
            r.ora.rounds(chunk - done)
            _compare_game(gpu, r.ora, r.slot, 0, chunk)
        done = chunk
    for r in oras:
        i = r.ora.info(0)
        print("slot", r.slot, "games finished", i["gamesFinished"], "rows per net", r.rows)
        assert i["gamesFinished"] >= 2, (r.slot, i)
        assert min(r.rows) > 0
    assert gpu.stats()["errors"] == 0
    gpu.close()
    net.close()


def test_routed_parity_7x7_policy_init(b2c32):
    """The NI = 4 instantiation, and the routing of the opening (policy-init) evaluations:
    each opening move is sampled from the net of the player who makes it."""
    X, Y, W, G, visits = 7, 7, 5, 8, 16
    play = dict(init_games_with_policy=1, policy_init_area_prop=0.04)
    net, fw = _forwards(X, Y, W, b2c32)
    gpu = _match(X, Y, W, G, visits, b2c32, **play)
    oras = [Routed(X, Y, W, s, visits, fw, **play) for s in [0, 1, 2, 5, 7]]
    done = 0
    for chunk in CHECKPOINTS:
        gpu.step(chunk - done)
        for r in oras:
            r.ora.rounds(chunk - done)
            _compare_game(gpu, r.ora, r.slot, 0, chunk)
        done = chunk
    for r in oras:
        print("slot", r.slot, "games finished", r.ora.info(0)["gamesFinished"], "rows per net", r.rows)
        assert min(r.rows) > 0
    # both colourings were played: slots of both parities, and a finished game in some slot
    assert sum(r.ora.info(0)["gamesFinished"] for r in oras) >= 1
    assert gpu.stats()["errors"] == 0
    gpu.close()
    net.close()


# ---------------------------------------------------------------------------------------
# 2. Records.

def _check_records_against(X, Y, W, header, moves, oras):
    by_key = {(int(h[0]), int(h[1])): i for i, h in enumerate(header)}
    checked = 0
    for r in oras:
        finished = r.ora.info(0)["gamesFinished"]
        for n in range(finished):
            assert (r.slot, n) in by_key, "no record of slot %d game %d" % (r.slot, n)
            i = by_key[(r.slot, n)]
            seen = r.moves_of[n]
            assert seen[-1] is None and None not in seen[:-1]
            assert header[i, 2] == len(seen), (r.slot, n, header[i], len(seen))
            got = [(int(c), int(d)) for c, d in moves[i, :len(seen) - 1]]
            assert got == seen[:-1], (r.slot, n)
            assert np.all(moves[i, len(seen):] == 0xFF)
            checked += 1
        assert (r.slot, finished) not in by_key  # and no record of a game still running
    assert checked >= 2 * len(oras)
    # the last move (not visible through the oracle's info), the winner and the colour: every
    # record replays legally on the device rules to its recorded winner
    _assert_records_replay(X, Y, W, header, moves)


def test_records_of_sampled_slots(ci1_run):
    header, moves = ci1_run["records"]
    assert len(header) == ci1_run["stats"]["games_finished"] > 0
    _check_records_against(ci1_run["X"], ci1_run["Y"], ci1_run["W"], header, moves, ci1_run["oras"])


def test_all_slots_replayed_evaluation_counts(b2c32):
    """G = 5, every slot replayed: the device's per-net evaluation counts are the rows the
    routed oracles handed to each net."""
    X, Y, W, G, visits, rounds = 5, 5, 4, 5, 24, 1500
    net, fw = _forwards(X, Y, W, b2c32)
    gpu = _match(X, Y, W, G, visits, b2c32)
    oras = [Routed(X, Y, W, s, visits, fw) for s in range(G)]
    recs = []
    for _ in range(0, rounds, 300):  # the record buffer holds 2 G games: drain twice a game length
        gpu.step(300)
        recs.append(gpu.drain_games())
    for r in oras:
        r.rounds_polled(rounds)
        _compare_game(gpu, r.ora, r.slot, 0, rounds)
    st = gpu.stats()
    assert st["errors"] == 0 and st["games_dropped"] == 0
    assert sum(st["nn_evals"]) == sum(r.ora.info(0)["nnEvals"] for r in oras)
    assert st["nn_evals"] == [sum(r.rows[n] for r in oras) for n in (0, 1)]
    assert max(st["nn_batch_peak"]) <= G and min(st["nn_batch_peak"]) > 0
    header, moves = np.concatenate([h for h, _ in recs]), np.concatenate([m for _, m in recs])
    assert len(header) == st["games_finished"]
    _check_records_against(X, Y, W, header, moves, oras)
    cand, base = gpu.score(header)
    assert cand + base == len(header)
    gpu.close()
    net.close()


# ---------------------------------------------------------------------------------------
# 3. Cap and cache on the device.

def test_batch_cap_and_caches(b2c32):
    """A cap that defers rows every round and a cache per net.  (That the two caches stay
    apart cannot be checked against the oracle, whose cache is single: it rests on the one
    netOf helper behind the compaction and every cache access -- DESIGN.md.)"""
    X, Y, W, G, visits, cap, rounds = 5, 5, 4, 64, 16, 24, 3000

    def run():
        gpu = _match(X, Y, W, G, visits, b2c32, ci=4, cache=12, cap=cap)
        recs = []
        for _ in range(6):
            gpu.step(rounds // 6)
            recs.append(gpu.drain_games())
        st = gpu.stats()
        gpu.close()
        h, m = np.concatenate([h for h, _ in recs]), np.concatenate([m for _, m in recs])
        # games that finish in one commit launch take their record places in any order
        order = np.lexsort((h[:, 1], h[:, 0]))
        return h[order], m[order], st

    h1, m1, st = run()
    h2, m2, st2 = run()
    assert st["errors"] == 0 and st["games_dropped"] == 0
    assert len(h1) == st["games_finished"] >= G
    np.testing.assert_array_equal(h1, h2)
    np.testing.assert_array_equal(m1, m2)
    assert st["nn_evals"] == st2["nn_evals"] and min(st["nn_evals"]) > 0  # both nets evaluated rows
    print("per-net peaks", st["nn_batch_peak"], "evals", st["nn_evals"])
    assert max(st["nn_batch_peak"]) <= cap
    _assert_records_replay(X, Y, W, h1, m1)


# ---------------------------------------------------------------------------------------
# 4. No rows and no interference.

def test_selfplay_unaffected_by_a_match_in_the_process(b2c32):
    kw = dict(num_games=16, max_visits=16, seed=5, node_cap=64, commit_interval=4, nn_cache_log2=8)

    def rows(with_match):
        sp = kc.Selfplay(5, 5, 4, **kw)
        sp.step(400)
        if with_match:
            m = _match(5, 5, 4, 16, 12, b2c32, ci=2, cache=8)
            m.step(400)
            st = m.stats()
            assert st["games_dropped"] == 0 and st["errors"] == 0 and st["moves"] > 0
            m.close()
        sp.step(400)
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
