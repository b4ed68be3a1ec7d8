"""Uncertainty weighting of playouts on the device.  The frozen oracle has no
such weighting, so with the setting on the device is checked against the host function
(kc.uncertainty_weight, the same detmath sequence) and against invariants of the dumped tree:
every node's own weight (dump word 21) is the weight of ITS position's short-term error logit
under one of the eight symmetries, and every parent's sums are the weighted sums of its
children's records plus its own evaluation.

5x5/4, the stand-in network, one slot, 64 visits and node_cap 256 unless stated."""
import ctypes
import os

import numpy as np
import pytest
import torch

import katacoffee_amd as kc
from katacoffee_amd import train
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED, VISITS, CAP, MAX_W = 11, 64, 256, 8.0
ON = dict(use_uncertainty=1)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _f32(words):
    return np.asarray(words, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def game_moves():
    """The first moves (policy positions) of an oracle self-play game: a legal line to cut
    query positions from."""
    ora = oracle.Selfplay(5, 5, 4, games=1, max_visits=24, node_cap=128, seed=SEED, slot_base=3)
    moves = []
    while len(moves) < 12:
        ora.rounds(1)
        i = ora.info(0)
        if i["movesMade"] > len(moves):
            assert i["gameNum"] == 0 and i["lastCell"] >= 0, i
            moves.append(i["lastDir"] * 25 + i["lastCell"])
    return moves


def _analysis(X=5, Y=5, W=4, slots=1, cache=0, visits=VISITS, unc=ON, model_path=None, precision="default", **over):
    over.setdefault("use_graph_search", 0)
    over.setdefault("root_num_symmetries_to_sample", 1)
    an = kc.Analysis(X, Y, W, num_slots=slots, seed=SEED, node_cap=CAP, nn_cache_log2=cache, query_capacity=8,
                     model_path=model_path, nn_precision=precision,
                     search=kc.default_analysis_params(max_visits=visits, **over))
    if unc is not None:
        an.set_uncertainty(**unc)
    return an


def _paths(nodes, edges):
    """The move path from the root to every node of a dumped tree (no graph search: one each)."""
    paths = {0: []}
    for i in range(len(nodes)):
        for j in range(int(nodes[i, 10] & 0xFFFF)):
            c, mv = int(edges[i, j, 0]), int(edges[i, j, 2])
            assert 0 < c < len(nodes) and c not in paths, "not a tree"
            paths[c] = paths[i] + [mv]
    assert len(paths) == len(nodes)
    return [paths[i] for i in range(len(nodes))]


def _replay(X, Y, W, lines):
    """The positions after each move list, replayed on the device rules: cells, the last five
    moves (most recent first), the player to move, finished flags."""
    n, A = len(lines), X * Y
    cells = np.zeros((n, A), np.uint8)
    hc, hd = np.full((n, 5), -1, np.int8), np.full((n, 5), 4, np.int8)
    pla, fin = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    for t in range(max(len(m) for m in lines)):
        on = np.array([i for i in range(n) if len(lines[i]) > t])
        assert np.all(fin[on] == 0)
        mv = np.array([lines[i][t] for i in on], np.int32)
        legal, _ = kc.rules_batch(X, Y, W, cells[on], hc[on, 0], hd[on, 0], pla[on])
        assert np.all(legal[np.arange(len(on)), mv] == 1), "illegal move at depth %d" % t
        oc, f, _, _, _, _ = kc.play_batch(X, Y, W, cells[on], hc[on, 0], hd[on, 0], pla[on], mv)
        cells[on], fin[on] = oc, f
        hc[on, 1:], hd[on, 1:] = hc[on, :4], hd[on, :4]
        hc[on, 0], hd[on, 0] = (mv % A).astype(np.int8), (mv // A).astype(np.int8)
        pla[on] = 3 - pla[on]
    return cells, hc, hd, pla, fin


def _eight_weights(X, Y, W, pos, forward, **params):
    """[n][8] f32: kc.uncertainty_weight of out[P+3] of each position under each symmetry."""
    cells, hc, hd, pla, _ = pos
    n, P = len(pla), 4 * X * Y
    out = np.zeros((n, 8), np.float32)
    for s in range(8):
        packed, _ = kc.encode_batch(X, Y, W, cells, hc, hd, pla, np.full(n, s, np.int32), want_planes=False)
        logit = forward(packed)[:, P + 3]
        out[:, s] = [kc.uncertainty_weight(float(x), **dict(ON, **params))[1] for x in logit]
    return out


def _fake(X, Y, W):
    return lambda packed: kc.fake_net(X, Y, W, packed)


def _check_weights(X, Y, W, base, nodes, edges, only=None):
    """Every expanded non-terminal node's word 21 is one of its own position's eight weights,
    bit for bit; a terminal node with n visits weighs n * max_weight.  Returns how many of
    each were checked (the root excluded from the first count)."""
    lines = [base + p for p in _paths(nodes, edges)]
    idx = list(range(len(nodes))) if only is None else only
    flags = nodes[:, 10] >> 24
    expanded = [i for i in idx if flags[i] & 1 and not flags[i] & 2]
    terminal = [i for i in idx if flags[i] & 2]
    pos = _replay(X, Y, W, [lines[i] for i in expanded])
    eight = _eight_weights(X, Y, W, pos, _fake(X, Y, W))
    assert len(np.unique(_bits(eight))) > 4 * len(expanded)  # the weights tell positions and symmetries apart
    for k, i in enumerate(expanded):
        assert nodes[i, 21] in _bits(eight[k]), (i, lines[i], _f32(nodes[i, 21:22])[0], eight[k])
    for i in terminal:
        n = int(nodes[i, 0])
        assert n >= 1 and nodes[i, 1] == _bits(np.float32(n * MAX_W)), (i, n, _f32(nodes[i, 1:2])[0])
        assert nodes[i, 2] == _bits(np.float32(n * MAX_W * MAX_W))
    return len([i for i in expanded if i != 0]), len(terminal)


def _run(an, queries):
    h, m = an.analyze(queries)
    st = an.stats()
    assert st["errors"] == 0 and np.all(h["status"] == kc.ANALYSIS_OK)
    return h, m


# ---------------------------------------------------------------------------------------
# 4. Off is off.

def test_off_is_off_and_late_setter_is_rejected(game_moves):
    q = [dict(id=5, moves=game_moves[:6])]
    out = []
    for unc in (None, dict(use_uncertainty=0, uncertainty_coeff=0.5, uncertainty_exponent=0.7)):
        an = _analysis(unc=unc, use_graph_search=1, root_num_symmetries_to_sample=2)
        h, m = _run(an, q)
        nodes, edges = an.game_tree(0, CAP)
        out.append((h.tobytes(), m.tobytes(), nodes.tobytes(), edges.tobytes()))
        assert np.all(nodes[:, 21:23] == 0)
        assert _f32(nodes[0, 1:2])[0] == h[0]["visits"] == VISITS  # every weight 1
        with pytest.raises(kc.CoffeeError, match="set_uncertainty"):
            an.set_uncertainty(**ON)
        an.close()
    assert out[0] == out[1]
    an = _analysis(unc=None)
    an.step(1)
    rc = kc.lib().coffee_analysis_set_uncertainty(an.h, ctypes.byref(kc.default_uncertainty_params(**ON)))
    assert rc == -1  # COFFEE_EINVAL
    an.close()
    sp = kc.Selfplay(5, 5, 4, num_games=2, max_visits=8, node_cap=64)
    sp.set_uncertainty(**ON)
    with pytest.raises(kc.CoffeeError, match="uncertainty_coeff"):
        sp.set_uncertainty(use_uncertainty=1, uncertainty_coeff=2.0)
    sp.step(1)
    with pytest.raises(kc.CoffeeError, match="first round"):
        sp.set_uncertainty(use_uncertainty=0)
    sp.close()


# ---------------------------------------------------------------------------------------
# 5. Every node's weight is the right position's.

def test_every_node_weight_is_its_own_position(game_moves):
    base = game_moves[:8]
    an = _analysis()
    _run(an, [dict(id=1, moves=base)])
    nodes, edges = an.game_tree(0, CAP)
    an.close()
    assert nodes[0, 0] == VISITS
    checked, terminals = _check_weights(5, 5, 4, base, nodes, edges)
    print("expanded non-root nodes checked: %d, terminal nodes: %d, nodes: %d" % (checked, terminals, len(nodes)))
    assert checked >= 30 and terminals >= 1


def test_every_node_weight_with_the_nn_cache(game_moves):
    """Two slots search the same position beside each other with a 2^10-entry cache: a hit
    takes the weight of the evaluation that filled the slot -- one of the eight."""
    base = game_moves[:8]
    an = _analysis(slots=2, cache=10)
    _run(an, [dict(id=1, moves=base, stream=1), dict(id=2, moves=base, stream=2)])
    st = an.stats()
    total = 0
    for slot in range(2):
        nodes, edges = an.game_tree(slot, CAP)
        assert nodes[0, 0] == VISITS
        total += len(nodes)
        checked, _ = _check_weights(5, 5, 4, base, nodes, edges)
        assert checked >= 30
    an.close()
    assert st["nn_evals"] < total  # some evaluations came from the cache


# ---------------------------------------------------------------------------------------
# 6. The sums are the reference's.

CANCEL_FLOOR = 0.1


def _check_sums(nodes, edges):
    """recomputeNodeStats / addLeafValue in float64 from the dump (value weighting and SVB off,
    no graph search: a child's weight in its parent is its own weight sum).  Plain relative
    tolerance 1e-5 on all five sums: f32 sums of at most 65 terms, 65 * 2^-24 = 4e-6.
    The one exception: a mean (utilityAvg, winLossAvg) whose terms of both signs cancel to
    less than CANCEL_FLOOR of their mean magnitude has lost more than a decimal digit to the
    cancellation -- a sum's rounding is relative to its terms, not to its result -- and is
    held to 1e-5 of that mean magnitude instead.  Returns the largest plain relative
    difference over the values held to the plain bound, the same over all values, the number
    of values under the floor, and the number of parents."""
    worst = worst_all = 0.0
    parents = cancelled = 0
    for i in range(len(nodes)):
        rec = _f32(nodes[i, 1:8]).astype(np.float64)  # ws, wsq, u, usq, wl, nnWin, nnLoss
        flags, k = int(nodes[i, 10] >> 24), int(nodes[i, 10] & 0xFFFF)
        if flags & 2 or not flags & 1:
            assert k == 0
            continue
        w = float(_f32(nodes[i, 21:22])[0])
        self_u = rec[5] - rec[6]
        kids = _f32(nodes[edges[i, :k, 0].astype(np.int64), 1:6]).astype(np.float64).reshape(k, 5)
        np.testing.assert_array_equal(edges[i, :k, 1], nodes[edges[i, :k, 0].astype(np.int64), 0])
        assert nodes[i, 0] == 1 + edges[i, :k, 1].sum()
        ws = kids[:, 0].sum() + w
        want = [ws, kids[:, 1].sum() + w * w,
                ((kids[:, 0] * kids[:, 2]).sum() + w * self_u) / ws,
                ((kids[:, 0] * kids[:, 3]).sum() + w * self_u * self_u) / ws,
                ((kids[:, 0] * kids[:, 4]).sum() + w * self_u) / ws]
        scale = [ws, want[1],
                 ((kids[:, 0] * np.abs(kids[:, 2])).sum() + w * abs(self_u)) / ws,
                 want[3],
                 ((kids[:, 0] * np.abs(kids[:, 4])).sum() + w * abs(self_u)) / ws]
        for name, got, wnt, sc in zip(["weightSum", "weightSqSum", "utilityAvg", "utilitySqAvg", "winLossAvg"],
                                      rec[:5], want, scale):
            rel = abs(got - wnt) / abs(wnt) if wnt != 0.0 else float(got != 0.0)
            worst_all = max(worst_all, rel)
            if abs(wnt) >= CANCEL_FLOOR * sc:
                worst = max(worst, rel)
                assert rel <= 1e-5, (i, name, got, wnt)
            else:
                cancelled += 1
                assert abs(got - wnt) <= 1e-5 * sc, (i, name, got, wnt, sc)
        parents += k > 0
    return worst, worst_all, cancelled, parents


def test_sums_are_the_weighted_sums(game_moves):
    base = game_moves[:8]
    an = _analysis(value_weight_exponent=0.0, subtree_value_bias_factor=0.0)
    h, _ = _run(an, [dict(id=1, moves=base)])
    nodes, edges = an.game_tree(0, CAP)
    an.close()
    worst, worst_all, cancelled, parents = _check_sums(nodes, edges)
    print("largest relative difference of a recomputed sum: %.3e (with the %d cancelling means: %.3e) over %d "
          "parents" % (worst, cancelled, worst_all, parents))
    assert parents >= 10 and cancelled < parents  # the exception stays the exception
    assert _bits(h[0]["weight_sum"]) == nodes[0, 1] and h[0]["weight_sum"] != h[0]["visits"]


def _child_weight(ev, cv, raw):
    return np.float32(raw) * (np.float32(ev) / np.float32(max(int(cv), 1)))


def _lcb_radius(lcb_stdevs, pla, cv, ws_raw, wsq_raw, u, usq, ev):
    """lcbAndRadius (getSelfUtilityLCBAndRadius searchhelpers.cpp:469-521) one float32 operation
    at a time, in the kernel's order (the restatement of tests/test_gpu_analysis.py)."""
    _f = np.float32
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


def test_default_search_settings_with_weighting_on(game_moves):
    """The analysis defaults (value weight exponent 0.5, SVB, graph search, LCB) with the
    setting on: no error, the root's weight is not its visit count, and the best move's
    report follows the report rules from the dumped child record."""
    params = kc.default_analysis_params(max_visits=VISITS)
    an = kc.Analysis(5, 5, 4, num_slots=1, seed=SEED, node_cap=CAP, query_capacity=2, search=params)
    an.set_uncertainty(**ON)
    h, m = _run(an, [dict(id=1, moves=game_moves[:8])])
    nodes, edges = an.game_tree(0, CAP)
    an.close()
    h, k = h[0], int(h[0]["num_children"])
    assert h["visits"] == VISITS == nodes[0, 0] and h["weight_sum"] != h["visits"]
    assert _bits(h["weight_sum"]) == nodes[0, 1]
    m = m[0][:k]
    best = int(np.nonzero(m["order"] == 0)[0][0])
    c = nodes[int(edges[0, best, 0])]
    assert m["move"][best] == edges[0, best, 2] and m["edge_visits"][best] == edges[0, best, 1]
    assert m["visits"][best] == c[0] and _bits(m["weight_sum"][best]) == c[1]
    assert _bits(m["utility_avg"][best]) == c[3] and _bits(m["win_loss_avg"][best]) == c[5]
    assert m["weight_sum"][best] != m["visits"][best]
    cf = _f32(c[1:5])
    lcb, radius = _lcb_radius(params.lcb_stdevs, int(h["pla"]), int(c[0]), cf[0], cf[1], cf[2], cf[3],
                              int(edges[0, best, 1]))
    assert _bits(m["lcb"][best]) == _bits(lcb) and _bits(m["radius"][best]) == _bits(radius)
    assert m["play_selection_value"][best] == m["play_selection_value"].max()


# ---------------------------------------------------------------------------------------
# 7. Wiring control.

def test_on_and_off_differ(game_moves):
    q = [dict(id=1, moves=game_moves[:8])]
    trees = []
    for unc in (dict(use_uncertainty=0), ON):
        an = _analysis(unc=unc)
        h, _ = _run(an, q)
        nodes, edges = an.game_tree(0, CAP)
        an.close()
        assert (h[0]["weight_sum"] == h[0]["visits"]) == (unc["use_uncertainty"] == 0)
        trees.append((nodes, edges))
    (n0, e0), (n1, e1) = trees
    assert n0.shape != n1.shape or not np.array_equal(n0[:, :11], n1[:, :11]) or not np.array_equal(e0, e1)
    assert np.all(n0[:, 21] == 0) and np.all(n1[(n1[:, 10] >> 24) & 1 == 1, 21] != 0)


# ---------------------------------------------------------------------------------------
# 8. Root symmetries = 4.

def test_root_weight_over_four_symmetries(game_moves):
    base = game_moves[:8]
    an = _analysis(root_num_symmetries_to_sample=4)
    _run(an, [dict(id=1, moves=base)])
    nodes, edges = an.game_tree(0, CAP)
    an.close()
    eight = _eight_weights(5, 5, 4, _replay(5, 5, 4, [base]), _fake(5, 5, 4))[0]
    w = _f32(nodes[0, 21:22])[0]
    assert eight.min() <= w <= eight.max(), (w, eight)
    assert nodes[0, 21] not in _bits(eight)  # the weight of an averaged error, not of one symmetry
    # below the root nothing changes: one symmetry per evaluation
    checked, _ = _check_weights(5, 5, 4, base, nodes, edges, only=list(range(1, len(nodes))))
    assert checked >= 30


# ---------------------------------------------------------------------------------------
# 9. Geometries: the four- and seven-item kernels.

def _legal_line(X, Y, W, n):
    """n legal moves from the empty board: each time the middle one of the legal moves."""
    line = []
    for _ in range(n):
        cells, hc, hd, pla, fin = _replay(X, Y, W, [line]) if line else (
            np.zeros((1, X * Y), np.uint8), np.full((1, 5), -1, np.int8), np.full((1, 5), 4, np.int8),
            np.ones(1, np.uint8), np.zeros(1, np.uint8))
        assert fin[0] == 0
        legal, _ = kc.rules_batch(X, Y, W, cells, hc[:, 0], hd[:, 0], pla)
        ok = np.nonzero(legal[0])[0]
        line.append(int(ok[len(ok) // 2]))
    return line


@pytest.mark.parametrize("X,Y,W", [(7, 7, 5), (9, 9, 5)], ids=["7x7", "9x9"])
def test_weights_at_wider_geometries(X, Y, W):
    base = _legal_line(X, Y, W, 3)
    an = _analysis(X, Y, W, visits=32, value_weight_exponent=0.0, subtree_value_bias_factor=0.0)
    h, _ = _run(an, [dict(id=1, moves=base)])
    nodes, edges = an.game_tree(0, CAP)
    an.close()
    k = int(nodes[0, 10] & 0xFFFF)
    assert nodes[0, 0] == 32 and k >= 4 and h[0]["weight_sum"] != 32
    checked, _ = _check_weights(X, Y, W, base, nodes, edges, only=[0] + [int(c) for c in edges[0, :k, 0]])
    assert checked >= 4
    # and every parent's sums, as in test 6, on the four- / seven-item computeLevel
    worst, worst_all, cancelled, parents = _check_sums(nodes, edges)
    print("%dx%d: largest relative difference %.3e (with the %d cancelling means: %.3e) over %d parents" %
          (X, Y, worst, cancelled, worst_all, parents))
    assert parents >= 3


# ---------------------------------------------------------------------------------------
# 10. Fused against separate rounds.

def _selfplay(fused, **kw):
    env = {"COFFEE_FUSED_ROUNDS": "1" if fused else "0"}
    old = {k: os.environ.pop(k, None) for k in env}
    os.environ.update(env)
    try:
        sp = kc.Selfplay(5, 5, 4, **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    sp.set_uncertainty(**ON)
    return sp


@pytest.mark.parametrize("ci", [3, 16])
def test_fused_rounds_match_separate_rounds_with_weighting(ci):
    G = 64
    kw = dict(num_games=G, max_visits=48, seed=61, node_cap=CAP, commit_interval=ci, nn_cache_log2=10)
    a, b = _selfplay(True, **kw), _selfplay(False, **kw)
    a.enable_timing(1)
    b.enable_timing(1)
    done = 0
    # 40 rounds: inside the first search; 1370: past the first finished games' rows and inside a
    # search at both intervals (a search takes 51 rounds, so the games move every 51 / 64 rounds)
    for chunk in [5, 40, 1370]:
        a.step(chunk - done)
        b.step(chunk - done)
        done = chunk
        weighted = 0
        for g in range(G):
            assert a.game_info(g) == b.game_info(g), (done, g)
            na, ea = a.game_tree(g, CAP)
            nb, eb = b.game_tree(g, CAP)
            np.testing.assert_array_equal(na, nb, err_msg="round %d game %d nodes" % (done, g))
            np.testing.assert_array_equal(ea, eb, err_msg="round %d game %d edges" % (done, g))
            weighted += len(na) > 0 and bool(np.any(na[:, 21] != 0))
        print("commit interval %d, round %d: %d of %d trees carry weights" % (ci, done, weighted, G))
        if done >= 40:  # (after 5 rounds a root may not have its evaluation yet)
            assert weighted > G // 2, (done, weighted)
    sa, sb = a.stats(), b.stats()
    assert sa["errors"] == 0 and sa["moves"] > 0
    for k in ("playouts", "nn_evals", "moves", "games_finished", "rows_pending"):
        assert sa[k] == sb[k], k
    ra, rb = a.drain_rows(), b.drain_rows()
    assert len(ra["meta"]) > 0
    oa = np.lexsort((ra["meta"][:, 2], ra["meta"][:, 1], ra["meta"][:, 0]))
    ob = np.lexsort((rb["meta"][:, 2], rb["meta"][:, 1], rb["meta"][:, 0]))
    for k in ra:
        np.testing.assert_array_equal(ra[k][oa], rb[k][ob], err_msg=k)
    assert a.kernel_time(4)[1] > 0 and b.kernel_time(4)[1] == 0  # fused launches ran in a only
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------
# 11. Match: one setting for both nets.

@pytest.fixture(scope="module")
def b2c32(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("unc") / "b2c32.cfnn")
    kc.write_random_model("b2c32", 0xBEEF, p)
    return p


def _records_replay(X, Y, W, header, moves):
    A = X * Y
    lines = [[int(moves[i, t, 1]) * A + int(moves[i, t, 0]) for t in range(int(header[i, 2]))]
             for i in range(len(header))]
    _, _, _, pla, fin = _replay(X, Y, W, lines)  # asserts every move legal when played
    for i in range(len(header)):
        if header[i, 3] != 0:
            assert fin[i] == 1 and header[i, 3] == 3 - pla[i], header[i]  # the last mover won


def test_match_weights_come_from_the_roots_own_net(b2c32):
    X, Y, W, A, P, G = 5, 5, 4, 25, 100, 8
    mt = kc.Match(X, Y, W, num_games=G, candidate_path=b2c32, seed=SEED, node_cap=128, nn_precision="accurate",
                  search=kc.default_match_params(max_visits=32))
    mt.set_uncertainty(**ON)
    net = kc.Network(b2c32, X, Y, W, precision="accurate")
    forwards = [_fake(X, Y, W), net.forward]
    seen = {0: set(), 1: set()}  # slots whose root each net evaluated and that were checked
    rounds = 0
    for turn in (0, 1):
        # until every slot searches its game-0 position of this turn
        while True:
            infos = [mt.game_info(g) for g in range(G)]
            if all(i["gameNum"] == 0 and i["turn"] == turn and i["phase"] == 1 for i in infos):
                break
            assert rounds < 80 and all(i["turn"] <= turn for i in infos), infos
            mt.step(1)
            rounds += 1
        for g, i in enumerate(infos):
            line = [] if turn == 0 else [i["lastDir"] * A + i["lastCell"]]
            which = 1 if i["pla"] == (1 if g % 2 == 0 else 2) else 0  # the candidate is black in even slots
            nodes, _ = mt.game_tree(g, 128)
            eight = _eight_weights(X, Y, W, _replay(X, Y, W, [line]), forwards[which])[0]
            other = _eight_weights(X, Y, W, _replay(X, Y, W, [line]), forwards[1 - which])[0]
            assert nodes[0, 21] in _bits(eight), (turn, g, which, _f32(nodes[0, 21:22])[0], eight)
            assert nodes[0, 21] not in _bits(other)
            seen[which].add(g)
    assert len(seen[0]) == G and len(seen[1]) == G
    net.close()
    recs = []
    for _ in range(8):
        mt.step(250)
        recs.append(mt.drain_games())
    st = mt.stats()
    header, moves = np.concatenate([h for h, _ in recs]), np.concatenate([m for _, m in recs])
    mt.close()
    assert st["errors"] == 0 and st["games_dropped"] == 0 and min(st["nn_evals"]) > 0
    assert len(header) >= G and len(header) == st["games_finished"]
    _records_replay(X, Y, W, header, moves)


# ---------------------------------------------------------------------------------------
# 12. Trained head end to end.

def test_trained_error_head_drives_the_weights(tmp_path, game_moves):
    sp = kc.Selfplay(5, 5, 4, num_games=64, max_visits=16, seed=5, node_cap=128, commit_interval=4)
    sp.step(600)
    rows = sp.drain_rows()
    sp.close()
    assert len(rows["meta"]) >= 256
    batch = train.rows_to_batch({k: rows[k][:512] for k in train.ROW_KEYS}, 5, 5)
    torch.manual_seed(0)
    net = train.CoffeeNet("b2c32")
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    for _ in range(20):
        train.train_step(net, opt, batch, st_error_weight=1.0)
    path = str(tmp_path / "trained.cfnn")
    train.save_cfnn(net, path)
    an = _analysis(slots=4, visits=48, model_path=path, precision="accurate", use_graph_search=1)
    h, _ = _run(an, [dict(id=i + 1, moves=game_moves[:t]) for i, t in enumerate([0, 3, 6, 9])])
    an.close()
    for r in h:
        assert r["visits"] == 48
        # w_min = 0 (err -> inf), the most a visit weighs is max_weight
        assert 0.0 <= r["weight_sum"] <= r["visits"] * MAX_W, r
        assert r["weight_sum"] != r["visits"]


# ---------------------------------------------------------------------------------------
# The commands: a config's keys reach the engine (`katago analysis` as the example; the three
# commands share the config layer and each hands its result to its engine's setter).

def _winrate(white_wl, pla):
    w = 0.5 * (max(-1.0, min(1.0, float(white_wl))) + 1.0)
    return w if pla == 2 else 1.0 - w


def test_analysis_command_reads_the_config_keys():
    import json
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [os.path.join(repo, "katacoffee_amd", "katago"), "analysis", "-config",
           os.path.join(repo, "configs", "analysis_coffee5.cfg"), "-override-config",
           "maxVisits=48,numAnalysisSlots=2,nnCacheSizePowerOfTwo=0,useUncertainty=true,uncertaintyCoeff=0.5,"
           "uncertaintyMaxWeight=4"]
    r = subprocess.run(cmd, input='{"id":"a","moves":[]}\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip())
    got = {}
    for on in (0, 1):
        an = kc.Analysis(5, 5, 4, num_slots=2, seed=1, search=kc.default_analysis_params(max_visits=48))
        an.set_uncertainty(use_uncertainty=on, uncertainty_coeff=0.5, uncertainty_max_weight=4.0)
        h, m = an.analyze([dict(id=1, moves=[])])
        an.close()
        k = int(h[0]["num_children"])
        best = m[0][:k][m[0][:k]["order"] == 0][0]
        got[on] = (_winrate(h[0]["win_loss_avg"], 1), int(best["move"]), int(best["edge_visits"]),
                   _winrate(best["win_loss_avg"], 1))
    top = out["moveInfos"][0]
    mv = (ord(top["move"][2]) - 97) * 25 + (ord(top["move"][1]) - 97) * 5 + (ord(top["move"][0]) - 97)
    assert got[0] != got[1]
    assert out["rootInfo"]["winrate"] == pytest.approx(got[1][0], abs=2e-6)
    assert (mv, top["visits"]) == got[1][1:3] and top["winrate"] == pytest.approx(got[1][3], abs=2e-6)
    assert out["rootInfo"]["winrate"] != pytest.approx(got[0][0], abs=2e-6)
    bad = subprocess.run(cmd[:-1] + ["useUncertainty=true,uncertaintyCoeff=7"], input="", capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode != 0 and "uncertaintyCoeff" in bad.stderr


def test_selfplay_and_gatekeeper_commands_set_the_weighting(tmp_path):
    """The other two commands hand the parsed keys to their engines' setters: both run to the
    end with the setting on and log the values the engine accepted; without the keys neither
    logs it.  (Their seeds are drawn at start, so there is no second run to compare with.)"""
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    katago = os.path.join(repo, "katacoffee_amd", "katago")
    keys = "useUncertainty=true,uncertaintyCoeff=0.5,uncertaintyExponent=0.5,uncertaintyMaxWeight=4"
    line = "coeff 0.5, exponent 0.5, max weight 4"
    models = tmp_path / "models"
    models.mkdir()
    kc.write_random_model("b2c32", 5, str(models / "b2c32-s0.cfnn"))
    for extra in ("," + keys, ""):
        out = tmp_path / ("out" + str(len(extra)))
        r = subprocess.run([katago, "selfplay", "-config", os.path.join(repo, "configs", "selfplay_coffee5.cfg"),
                            "-models-dir", str(models), "-output-dir", str(out), "-max-games-total", "8",
                            "-override-config", "numGameThreads=16,maxVisits=8,maxRowsPerTrainFile=100" + extra],
                           capture_output=True, text=True, timeout=120)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log
        assert ("uncertainty weighting on: " + line in log) == bool(extra), log
        assert "gpu 0.0 done" in log
    for k in ("test", "accepted"):
        (tmp_path / k).mkdir()
    kc.write_random_model("b2c32", 21, str(tmp_path / "accepted" / "base-s0.cfnn"))
    kc.write_random_model("b2c32", 22, str(tmp_path / "test" / "cand-s1.cfnn"))
    r = subprocess.run([katago, "gatekeeper", "-config", os.path.join(repo, "configs", "gatekeeper_coffee5.cfg"),
                        "-test-models-dir", str(tmp_path / "test"), "-accepted-models-dir", str(tmp_path / "accepted"),
                        "-rejected-models-dir", str(tmp_path / "rejected"), "-sgf-output-dir", str(tmp_path / "sgf"),
                        "-quit-if-no-nets-to-test", "-no-autoreject-old-models", "-override-config",
                        "numGamesPerGating=4,numGameThreads=4,maxVisits=8," + keys],
                       capture_output=True, text=True, timeout=120)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log
    assert "uncertainty weighting on for both nets: " + line in log, log
    assert "candidate cand-s1 accepted" in log or "candidate cand-s1 rejected" in log, log
