"""Batched position analysis on the device (kc.Analysis): loaded positions are searched
exactly as the CPU oracle searches them in a game, the report equals the tree it was made
from, the best move is the move self-play plays, slots refill without affecting each other,
and bad or terminal queries are answered without a search.

Everything is 5x5/4 with the stand-in network, NN cache off, 24 visits and node_cap 128
unless stated."""
import numpy as np
import pytest

import katacoffee_amd as kc
from oracle import oracle

pytestmark = pytest.mark.gpu

INFO_KEYS = [("phase", "phase"), ("rootK", "rootK"), ("liveCount", "nodeCount"), ("gameNum", "gameNum"),
             ("turn", "turn"), ("pla", "pla"), ("playouts", "playouts"), ("nnEvals", "nnEvals"),
             ("moves", "movesMade"), ("gamesFinished", "gamesFinished"), ("rngCtr", "rngCtr"),
             ("lastCell", "lastCell"), ("lastDir", "lastDir")]
# counters that run over a slot's (an oracle game slot's) whole life: compared as the increase
# since the position was loaded (reached) -- an analysis slot cannot know a game's earlier playouts
RUNNING = ("playouts", "nnEvals")
SEED, VISITS, CAP = 11, 24, 128
INLINE_EDGES = 16  # child slots stored with a node; the rest live in the edge pool


def _oracle(X, Y, W, seed=SEED, slot=3):
    return oracle.Selfplay(X, Y, W, games=1, max_visits=VISITS, node_cap=CAP, seed=seed, slot_base=slot)


def _oracle_to_turn(ora, A, moves, turn):
    """Steps the oracle one round at a time until `turn` moves are made, appending every move
    that appears in info to `moves` (policy positions)."""
    while ora.info(0)["movesMade"] < turn:
        ora.rounds(1)
        i = ora.info(0)
        if i["movesMade"] > len(moves):
            assert i["movesMade"] == len(moves) + 1 and i["gameNum"] == 0 and i["lastCell"] >= 0
            moves.append(i["lastDir"] * A + i["lastCell"])
    i = ora.info(0)
    # after a commit: the next search has not begun
    assert i["phase"] == 0 and i["rootK"] == 0 and i["nodeCount"] == 0 and i["turn"] == turn
    return i


def _paired_search(X, Y, W, turns, rounds=26):
    """The oracle's game of global slot 3 beside a one-slot analysis engine with the oracle's
    parameters: at each of `turns` the position is submitted with the oracle's RNG counter and
    both are stepped `rounds` rounds, compared after every one."""
    A = X * Y
    ora = _oracle(X, Y, W)
    an = kc.Analysis(X, Y, W, num_slots=1, seed=SEED, node_cap=CAP, query_capacity=4,
                     search=kc.default_search_params(max_visits=VISITS))
    moves = []
    for n, turn in enumerate(turns):
        oi0 = _oracle_to_turn(ora, A, moves, turn)
        gi0 = an.game_info(0)
        assert an.submit([dict(id=n + 1, moves=moves, max_visits=VISITS, stream=3, game_num=0,
                               rng_counter=oi0["rngCtr"])]) == 1
        for r in range(1, rounds + 1):
            ora.rounds(1)
            an.step(1)
            gi, oi = an.game_info(0), ora.info(0)
            for a, b in INFO_KEYS:
                if a in RUNNING:
                    assert gi[a] - gi0[a] == oi[b] - oi0[b], (turn, r, a, gi[a] - gi0[a], oi[b] - oi0[b])
                else:
                    assert gi[a] == oi[b], (turn, r, a, gi[a], oi[b])
            gn, ge = an.game_tree(0)
            on, oe = ora.game_tree(0)
            np.testing.assert_array_equal(gn, on, err_msg="turn %d round %d nodes" % (turn, r))
            np.testing.assert_array_equal(ge, oe, err_msg="turn %d round %d edges" % (turn, r))
            if gi["phase"] == 1:
                np.testing.assert_array_equal(an.root_policy(0), ora.root_noised(0))
        # The oracle commits in the round its root reaches the limit, so its 24-visit tree
        # cannot be observed: the last compared round has 23 root visits.
        assert gn[0, 0] == VISITS - 1 and len(moves) == turn
        an.step(1)  # the 24th visit: reported, the slot idle again
        h, _ = an.drain()
        assert len(h) == 1 and h[0]["id"] == n + 1 and h[0]["status"] == kc.ANALYSIS_OK
        assert h[0]["visits"] == VISITS and h[0]["turn"] == turn
    st = an.stats()
    assert st["errors"] == 0 and st["queries_loaded"] == len(turns) == st["queries_finished"]
    an.close()
    return moves


# ---------------------------------------------------------------------------------------
# 1. Search from a loaded position equals the oracle's search of it, bit for bit.

def test_loaded_search_equals_oracle_5x5():
    moves = _paired_search(5, 5, 4, [0, 1, 5, 12])
    assert len(moves) == 12


def test_loaded_search_equals_oracle_7x7():
    _paired_search(7, 7, 5, [3])  # P = 196: the four-item kernels


# ---------------------------------------------------------------------------------------
# 2. Report equals the tree.

def _f(x):
    return np.float32(x)


def _child_weight(ev, cv, raw):
    return _f(raw) * (_f(ev) / _f(max(int(cv), 1)))


def _lcb_radius(lcb_stdevs, pla, cv, ws_raw, wsq_raw, u, usq, ev):
    """lcbAndRadius (getSelfUtilityLCBAndRadius searchhelpers.cpp:469-521) one float32
    operation at a time, in the kernel's order."""
    radius = _f(2.0) * _f(1.0) * _f(lcb_stdevs)
    lcb = -radius
    ws, wsq = _child_weight(ev, cv, ws_raw), _child_weight(ev, cv, wsq_raw)
    if cv == 0 or ws <= 0 or wsq <= 0:
        return lcb, radius
    u, usq = _f(u), _f(usq)
    ess = (ws * ws) / wsq
    prior_weight = ws / ((ess * ess) * ess)
    usq = max(usq, u * u + _f(1e-8))
    usq = (usq * ws + (usq + _f(1.0)) * prior_weight) / (ws + prior_weight)
    ws = ws + prior_weight
    wsq = wsq + prior_weight * prior_weight
    ess = (ws * ws) / wsq
    self_u = u if pla == 2 else -u
    variance = usq - u * u
    stdev = np.sqrt(_f(variance / ess))
    radius = stdev * _f(lcb_stdevs)
    return self_u - radius, radius


def _walk_pv(nodes, edges, child_slot, max_len):
    """The stated rule on the dump: the child's move, then at every node the child with the
    most edge visits (ties: lower slot), until a node without children or a terminal node."""
    node, mv = int(edges[0, child_slot, 0]), int(edges[0, child_slot, 2])
    pv = []
    while len(pv) < max_len:
        pv.append(mv)
        k, flags = int(nodes[node, 10] & 0xFFFF), int(nodes[node, 10] >> 24)
        if k == 0 or flags & 2:
            break
        best = int(np.argmax(edges[node, :k, 1]))  # the first maximum
        node, mv = int(edges[node, best, 0]), int(edges[node, best, 2])
    return pv


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _check_report(X, Y, W, seed, turn, max_pv_len=16, visits=VISITS):
    A, P = X * Y, 4 * X * Y
    ora = _oracle(X, Y, W, seed=seed)
    moves = []
    oi = _oracle_to_turn(ora, A, moves, turn)
    ora.rounds(8)  # past the root evaluation: the oracle's root now holds its NN policy
    onodes = ora.nodes(0)
    root_policy = onodes["policy"][ora.info(0)["rootIdx"]]
    params = kc.default_search_params(max_visits=visits)
    an = kc.Analysis(X, Y, W, num_slots=1, seed=seed, node_cap=CAP, query_capacity=2, max_pv_len=max_pv_len,
                     search=params)
    h, m = an.analyze([dict(id=77, moves=moves, stream=3, rng_counter=oi["rngCtr"])], rounds_per_step=9)
    # one query: the idle slot keeps the tree the report was made from
    nodes, edges = an.game_tree(0)
    st = an.stats()
    an.close()
    assert st["errors"] == 0 and st["queries_finished"] == 1
    h, m = h[0], m[0]
    assert h["id"] == 77 and h["status"] == kc.ANALYSIS_OK and h["turn"] == turn and h["pla"] == 1 + turn % 2
    root = nodes[0]
    k = int(root[10] & 0xFFFF)
    assert h["visits"] == root[0] == visits and h["num_children"] == k
    assert max(m["pv_len"][:k]) > 1
    if visits > VISITS:
        assert k > INLINE_EDGES  # the root's edge-pool block is read
    for name, word in [("weight_sum", 1), ("utility_avg", 3), ("win_loss_avg", 5), ("nn_win", 6), ("nn_loss", 7)]:
        assert _bits(h[name]) == root[word], name
    assert np.all(m[k:].view(np.uint8) == 0)
    m = m[:k]
    np.testing.assert_array_equal(m["move"].astype(np.uint32), edges[0, :k, 2])
    np.testing.assert_array_equal(m["edge_visits"], edges[0, :k, 1])
    child = nodes[edges[0, :k, 0].astype(np.int64)]
    np.testing.assert_array_equal(m["visits"], child[:, 0])
    for name, word in [("weight_sum", 1), ("utility_avg", 3), ("win_loss_avg", 5)]:
        np.testing.assert_array_equal(_bits(m[name]), child[:, word], err_msg=name)
    # the root's NN policy before temperature and noise, from the oracle's search of the position
    np.testing.assert_array_equal(_bits(m["prior"]), _bits(root_policy[m["move"]]))
    pla = int(h["pla"])
    for i in range(k):
        assert list(m["pv"][i][:m["pv_len"][i]]) == _walk_pv(nodes, edges, i, max_pv_len), i
        assert np.all(m["pv"][i][m["pv_len"][i]:] == 0)
        lcb, radius = _lcb_radius(params.lcb_stdevs, pla, int(child[i, 0]), child[i, 1:2].view(np.float32)[0],
                                  child[i, 2:3].view(np.float32)[0], child[i, 3:4].view(np.float32)[0],
                                  child[i, 4:5].view(np.float32)[0], int(edges[0, i, 1]))
        assert _bits(m["lcb"][i]) == _bits(lcb) and _bits(m["radius"][i]) == _bits(radius), \
            (i, m["lcb"][i], lcb, m["radius"][i], radius)
    # order: a permutation, sorted by play-selection value descending, ties by child slot
    assert sorted(m["order"]) == list(range(k))
    by_order = np.argsort(m["order"])
    keys = [(-float(m["play_selection_value"][i]), int(i)) for i in by_order]
    assert keys == sorted(keys)


def test_report_equals_tree_5x5_empty_board():
    _check_report(5, 5, 4, SEED, 0)


def test_report_equals_tree_5x5_wide_root():
    """24 visits give the empty board's root 11 children (measured), not more than 16: at 48
    it has 20, so the children past the 16 stored with the node come from the edge pool."""
    _check_report(5, 5, 4, SEED, 0, visits=48)


def test_report_equals_tree_5x5_deep_lines():
    _check_report(5, 5, 4, SEED, 5)


def test_report_equals_tree_short_pv():
    _check_report(5, 5, 4, SEED, 2, max_pv_len=2)


def test_report_equals_tree_9x9():
    _check_report(9, 9, 5, SEED, 0)  # P = 324: the seven-item (widest) report kernel


# ---------------------------------------------------------------------------------------
# 3. Best move equals what self-play then plays.

def test_best_move_is_selfplays_move():
    X, Y, W, A = 5, 5, 4, 25
    over = dict(chosen_move_temperature=0.0, chosen_move_temperature_early=0.0)
    sp = kc.Selfplay(X, Y, W, num_games=1, max_visits=VISITS, seed=SEED, node_cap=CAP, **over)
    want = [0, 1, 4, 7]
    # polled after every round: a commit shows the new position, its last move and the RNG
    # counter the next search starts from
    moves, counter = [], {0: sp.game_info(0)["rngCtr"]}
    while len(moves) <= max(want):
        sp.step(1)
        info = sp.game_info(0)
        if info["moves"] > len(moves):
            assert info["moves"] == len(moves) + 1 and info["gameNum"] == 0 and info["lastCell"] >= 0
            moves.append(info["lastDir"] * A + info["lastCell"])
            assert info["phase"] == 0 and info["rootK"] == 0
            counter[len(moves)] = info["rngCtr"]
    sp.close()
    cases = [(t, moves[:t], counter[t], moves[t]) for t in want]
    an = kc.Analysis(X, Y, W, num_slots=2, seed=SEED, node_cap=CAP,
                     search=kc.default_search_params(max_visits=VISITS, use_lcb_for_selection=0, **over))
    h, m = an.analyze([dict(id=i, moves=c[1], stream=0, game_num=0, rng_counter=c[2]) for i, c in enumerate(cases)])
    assert an.stats()["errors"] == 0
    an.close()
    for i, c in enumerate(cases):
        k = h[i]["num_children"]
        assert h[i]["status"] == kc.ANALYSIS_OK and h[i]["visits"] == VISITS
        best = m[i][:k][m[i][:k]["order"] == 0]
        assert len(best) == 1 and best[0]["move"] == c[3], (c[0], best["move"], c[3])


# ---------------------------------------------------------------------------------------
# 4. Refill, and independence from neighbours.

@pytest.fixture(scope="module")
def two_games():
    out = []
    for seed in (SEED, SEED + 1):
        ora, moves = _oracle(5, 5, 4, seed=seed), []
        _oracle_to_turn(ora, 25, moves, 10)
        out.append(moves)
    return out


def test_refill_and_independence(two_games):
    queries = [dict(id=1000 + i, moves=two_games[i % 2][:i // 2], max_visits=[8, 24, 40][i % 3]) for i in range(19)]
    params = kc.default_analysis_params(max_visits=VISITS)
    an = kc.Analysis(5, 5, 4, num_slots=4, seed=SEED, node_cap=CAP, query_capacity=32, search=params)
    assert an.submit(queries) == 19
    got, order = {}, []
    for _ in range(400):
        an.step(7)
        h, m = an.drain()
        for i in range(len(h)):
            assert int(h[i]["id"]) not in got  # every id exactly once
            got[int(h[i]["id"])] = (h[i].tobytes(), m[i].tobytes(), int(h[i]["visits"]))
            order.append(int(h[i]["id"]))
        if len(got) == 19:
            break
    assert sorted(got) == [q["id"] for q in queries]
    assert order != sorted(order)  # the visit limits differ: not the submit order
    st = an.stats()
    assert st["queries_loaded"] == 19 and st["queries_finished"] == 19 and st["queries_rejected"] == 0
    assert st["errors"] == 0
    an.step(3)  # idle slots: nothing more comes out
    assert len(an.drain()[0]) == 0
    an.close()
    alone = kc.Analysis(5, 5, 4, num_slots=1, seed=SEED, node_cap=CAP, query_capacity=1, search=params)
    for q in queries:
        h, m = alone.analyze([q], rounds_per_step=11)
        assert got[q["id"]][2] == q["max_visits"]
        assert h[0].tobytes() == got[q["id"]][0], q["id"]
        assert m[0].tobytes() == got[q["id"]][1], q["id"]
    alone.close()


def test_submit_respects_query_capacity(two_games):
    an = kc.Analysis(5, 5, 4, num_slots=2, seed=SEED, node_cap=CAP, query_capacity=3,
                     search=kc.default_analysis_params(max_visits=8))
    queries = [dict(id=i + 1, moves=two_games[0][:i]) for i in range(5)]
    assert an.submit(queries) == 3
    assert an.submit(queries[3:]) == 0  # capacity is freed by drain, not by finishing
    an.step(40)
    assert an.submit(queries[3:]) == 0
    h, _ = an.drain()
    assert sorted(h["id"]) == [1, 2, 3]
    assert an.submit(queries[3:]) == 2
    an.step(40)
    h, _ = an.drain()
    assert sorted(h["id"]) == [4, 5] and np.all(h["status"] == kc.ANALYSIS_OK)
    an.close()


# ---------------------------------------------------------------------------------------
# 5. Bad and terminal queries.

def _special_move_lists(X, Y, W):
    """Found by replaying on the device rules (kc.rules_batch / kc.play_batch): a move onto an
    occupied cell, a move that breaks the previous move's direction restriction (both at index
    1), and a random legal game that ends with a win (its winner)."""
    A, n = X * Y, 64
    rng = np.random.default_rng(5)
    cells = np.zeros((n, A), np.uint8)
    lc, ld = np.full(n, -1, np.int8), np.full(n, 4, np.int8)
    pla = np.ones(n, np.uint8)
    lists = [[] for _ in range(n)]
    occupied = restricted = won = None
    for t in range(A):
        legal, has = kc.rules_batch(X, Y, W, cells, lc, ld, pla)
        assert np.all(has == 1)
        if t == 1:
            first = lists[0][0]
            bad = np.nonzero(legal[0] == 0)[0]
            on_stone = [int(p) for p in bad if p % A == first % A]
            off_line = [int(p) for p in bad if p % A != first % A]
            assert on_stone and off_line
            occupied, restricted = [first, on_stone[0]], [first, off_line[0]]
        mv = np.array([rng.choice(np.nonzero(legal[i])[0]) for i in range(n)], np.int32)
        oc, fin, win, _, _, _ = kc.play_batch(X, Y, W, cells, lc, ld, pla, mv)
        for i in range(n):
            lists[i].append(int(mv[i]))
        done = np.nonzero((fin == 1) & (win != 0))[0]
        if len(done):
            won = (lists[int(done[0])], int(win[done[0]]))
            assert won[1] == int(pla[done[0]])  # the mover wins
            break
        keep = np.nonzero(fin == 0)[0]
        assert len(keep) > 0
        cells, lc, ld = oc[keep], (mv[keep] % A).astype(np.int8), (mv[keep] // A).astype(np.int8)
        pla = (3 - pla[keep]).astype(np.uint8)
        lists = [lists[i] for i in keep]
        n = len(keep)
    assert won is not None
    return occupied, restricted, won


@pytest.mark.parametrize("X,Y,W", [(5, 5, 4), (6, 4, 3)], ids=["5x5", "6x4"])
def test_bad_and_terminal_queries(X, Y, W):
    occupied, restricted, (winning, winner) = _special_move_lists(X, Y, W)
    an = kc.Analysis(X, Y, W, num_slots=1, seed=SEED, node_cap=CAP, query_capacity=8,
                     search=kc.default_analysis_params(max_visits=VISITS))
    before = an.stats()
    assert an.submit([dict(id=1, moves=occupied), dict(id=2, moves=restricted), dict(id=3, moves=winning),
                      dict(id=4, moves=winning + [winning[0]])]) == 4
    an.step(0)  # loads only: these need no round
    h, m = an.drain()
    st = an.stats()
    assert list(h["id"]) == [1, 2, 3, 4]
    assert list(h["status"]) == [kc.ANALYSIS_ILLEGAL_MOVE, kc.ANALYSIS_ILLEGAL_MOVE, kc.ANALYSIS_GAME_OVER,
                                 kc.ANALYSIS_ILLEGAL_MOVE]
    assert list(h["info"]) == [1, 1, winner, len(winning)]
    assert h[2]["turn"] == len(winning) and np.all(h["num_children"] == 0) and np.all(m.view(np.uint8) == 0)
    assert st["rounds"] == before["rounds"] and st["playouts"] == before["playouts"] == 0
    assert st["nn_evals"] == 0 and st["errors"] == 0
    assert st["queries_loaded"] == 4 == st["queries_finished"] == st["queries_rejected"]
    # the slot serves the next query
    h, m = an.analyze([dict(id=9, moves=winning[:-1])])
    assert h[0]["status"] == kc.ANALYSIS_OK and h[0]["visits"] == VISITS and h[0]["turn"] == len(winning) - 1
    k = h[0]["num_children"]
    assert k > 0
    st = an.stats()
    assert st["errors"] == 0 and st["queries_finished"] == 5 and st["queries_rejected"] == 4
    an.close()
