"""Wide root noise and futile-visit pruning on the device.  The frozen oracle knows
neither rule, so with them on the device is checked against a restatement made from the dumped
trees: every root selection of a search is recomputed from the tree before it in np.float32, in
the kernel's operation order, with kc.wide_root_noise for the draws and kc.futile_visits for the
predicate (both the kernels' own header code on the host, pinned to float64 in
tests/test_root_search.py), and the child taken or the move expanded must be the one it names.
Off, nothing changes.

5x5/4, the stand-in network, one analysis slot, 64 visits, node cap 256, no graph search, one
root symmetry and no NN cache unless stated."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc
from oracle import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, VISITS, CAP = 11, 64, 256
_f = np.float32
FLT_MAX = np.finfo(np.float32).max
PRUNE = dict(use_noise_pruning=1, noise_prune_utility_scale=0.15)
FACTOR = dict(cpuct_utility_stdev_scale=0.85, cpuct_utility_stdev_prior=0.40, cpuct_utility_stdev_prior_weight=2.0)
BOTH = dict(PRUNE, **FACTOR)  # the two mechanisms of DESIGN.md 8g
NOISE = dict(root_noise_enabled=1)
WIDE = dict(wide_root_noise=0.5)
FUTILE = dict(futile_visits_threshold=0.4)
# the restatement's own limits (it holds the kernel's sequence for these settings only)
PLAIN = dict(cpuct_exploration_log=0.0, fpu_parent_weight_by_visited_policy_pow=2.0)


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


def _analysis(X=5, Y=5, W=4, visits=VISITS, rs=None, expl=None, cap=CAP, slots=1, **over):
    over.setdefault("use_graph_search", 0)
    over.setdefault("root_num_symmetries_to_sample", 1)
    params = kc.default_analysis_params(max_visits=visits, **dict(PLAIN, **over))
    an = kc.Analysis(X, Y, W, num_slots=slots, seed=SEED, node_cap=cap, nn_cache_log2=0, query_capacity=8,
                     search=params)
    if expl is not None:
        an.set_exploration(**expl)
    if rs is not None:
        an.set_root_search(**rs)
    return an, params


def _run(an, queries):
    h, m = an.analyze(queries)
    st = an.stats()
    assert st["errors"] == 0 and np.all(h["status"] == kc.ANALYSIS_OK)
    return h, m


def _root_dump(eng, slot, P):
    """The root and its children of a slot's tree (the export is breadth-first: the root, then its
    children in slot order), with the root's noised policy and the slot's game state."""
    nodes, edges = eng.game_tree(slot, P + 1)
    return dict(nodes=nodes, edges=edges, root_policy=eng.root_policy(slot), info=eng.game_info(slot))


# ---------------------------------------------------------------------------------------
# The restatement.

def _tree_sum64(v):
    """treeSum64 (oracle/ora_math.h) in np.float32: lane partials in order, then the xor butterfly."""
    s = np.zeros(64, np.float32)
    for l in range(64):
        a = _f(v[l]) if l < len(v) else _f(0)
        for j in range(l + 64, len(v), 64):
            a = _f(a + _f(v[j]))
        s[l] = a
    off = 32
    while off >= 1:
        s = (s + s[np.arange(64) ^ off]).astype(np.float32)
        off >>= 1
    return _f(s[0])


def _child_weight(ev, cv, raw):
    return _f(raw) * (_f(ev) / _f(max(int(cv), 1)))


def _stdev_factor(visits, ws, u, usq_avg, prior, pw, scale):
    """exploreStdevFactor (csrc/explore.h) one np.float32 operation at a time."""
    prior, pw, scale, ws, u, usq_avg = _f(prior), _f(pw), _f(scale), _f(ws), _f(u), _f(usq_avg)
    if scale == 0:
        return _f(1)
    if visits <= 0 or ws <= _f(1):
        stdev = prior
    else:
        usq = _f(u * u)
        usq_a = usq if usq_avg < usq else usq_avg
        var = _f(_f(_f(_f(_f(usq + _f(prior * prior)) * pw) + _f(usq_a * ws)) / _f(_f(pw + ws) - _f(1))) - usq)
        stdev = np.sqrt(_f(0) if var < 0 else var)
    return _f(_f(1) + _f(scale * _f(_f(stdev / prior) - _f(1))))


def _root_select(d, sp, rs, key, visit_limit, P, expl=None):
    """selectBest (search.hip; selectBestChildToDescend searchexplorehelpers.cpp:304-451) at the
    root of a dump in np.float32, in the kernel's operation order, with both root-search rules:
    futile first, then the desired-per-child funnel, then the noise.  key: (engine seed, global
    slot or stream, game number) of the stream the draws belong to.  Returns (slot, new move or -1,
    number of futile moves among the children and the candidate); slot == numChildren: a new child."""
    nodes, edges, pol = d["nodes"], d["edges"], d["root_policy"]
    wide, thr = float(rs.get("wide_root_noise", 0.0)), float(rs.get("futile_visits_threshold", 0.0))
    k = int(nodes[0, 10] & 0xFFFF)
    pla = int(nodes[0, 10] >> 16) & 0xFF
    visits = int(nodes[0, 0])
    turn = d["info"]["turn"]
    rec = _f32(nodes[0, 1:8])  # ws, wsq, u, usq, wl, nnWin, nnLoss
    moves = edges[0, :k, 2].astype(np.int64)
    p = pol[moves].astype(np.float32)
    ci = edges[0, :k, 0].astype(np.int64)
    np.testing.assert_array_equal(ci, np.arange(1, k + 1))
    cvis = nodes[ci, 0]
    cws, cu = _f32(nodes[ci, 1]), _f32(nodes[ci, 3])
    probs = [_f(0) if p[j] < 0 else p[j] for j in range(k)]
    cw = [_f(0) if p[j] < 0 else _child_weight(edges[0, j, 1], cvis[j], cws[j]) for j in range(k)]
    prob_mass, total = _tree_sum64(probs), _tree_sum64(cw)
    # fpuValue
    parent_u = rec[2]
    for_fpu = parent_u
    if sp.fpu_parent_weight_by_visited_policy:
        assert sp.fpu_parent_weight_by_visited_policy_pow == 2.0
        avg_w = min(_f(1), _f(prob_mass * prob_mass))
        for_fpu = _f(_f(avg_w * parent_u) + _f(_f(_f(1) - avg_w) * _f(rec[5] - rec[6])))
    reduction = _f(_f(sp.root_fpu_reduction_max) * np.sqrt(prob_mass))
    fpu = _f(for_fpu - reduction) if pla == 2 else _f(for_fpu + reduction)
    loss_value = _f(-1) if pla == 2 else _f(1)
    fpu = _f(fpu + _f(_f(loss_value - fpu) * _f(sp.root_fpu_loss_prop)))
    # exploreScaling and the stdev factor
    assert sp.cpuct_exploration_log == 0.0
    scaling = _f(_f(sp.cpuct_exploration) * np.sqrt(_f(total + _f(0.01))))
    if expl is not None:
        scaling = _f(scaling * _stdev_factor(visits, rec[0], rec[2], rec[3], expl["cpuct_utility_stdev_prior"],
                                             expl["cpuct_utility_stdev_prior_weight"],
                                             expl["cpuct_utility_stdev_scale"]))
    max_w = max([_f(0)] + cw)
    left = visit_limit - visits
    n_futile = 0

    def noised(u, prior, pos):
        if not wide > 0:
            return u, prior
        sm, bonus = kc.wide_root_noise(key[0], key[1], key[2], turn, visits, pos, prior, wide_root_noise=wide)
        return (_f(u + bonus) if pla == 2 else _f(u - bonus)), sm

    best, best_slot = -np.inf, -1
    coeff = _f(sp.root_desired_per_child_visits_coeff)
    for j in range(k):
        if p[j] < 0:
            continue
        w = cw[j]
        u = fpu if (cvis[j] == 0 or w <= 0) else cu[j]
        if thr > 0 and kc.futile_visits(max_w, rec[0], visits, left, int(edges[0, j, 1]), int(cvis[j]), w,
                                        futile_visits_threshold=thr):  # (before the funnel)
            val = -FLT_MAX
            n_futile += 1
        elif coeff > 0 and p[j] > 0 and w < np.sqrt(_f(_f(p[j] * total) * coeff)):
            val = _f(1e20)
        else:
            u, pj = noised(u, p[j], int(moves[j]))
            val = _f(_f(_f(scaling * pj) / _f(_f(1) + w)) + (u if pla == 2 else -u))
        if val > best:
            best, best_slot = val, j
    bp, bpos = _f(-1), -1
    has = np.zeros(P, bool)
    has[moves] = True
    for pos in range(P):
        if not has[pos] and pol[pos] >= 0 and pol[pos] > bp:
            bp, bpos = pol[pos], pos
    new_pos = -1
    if bpos >= 0:
        if thr > 0 and kc.futile_visits(max_w, rec[0], visits, left, is_new=True, futile_visits_threshold=thr):
            val = -FLT_MAX
            n_futile += 1
        else:
            u, bp = noised(fpu, bp, bpos)
            val = _f(_f(_f(scaling * bp) / _f(1)) + (u if pla == 2 else -u))
        if val > best:
            best_slot, new_pos = k, bpos
    return best_slot, new_pos, n_futile


def _taken(prev, cur):
    """The root's choice in the playout between two dumps one root visit apart: (slot, new move or
    -1)."""
    k = int(prev["nodes"][0, 10] & 0xFFFF)
    k_now = int(cur["nodes"][0, 10] & 0xFFFF)
    np.testing.assert_array_equal(cur["edges"][0, :k, 2], prev["edges"][0, :k, 2])
    rose = [s for s in range(k) if cur["edges"][0, s, 1] > prev["edges"][0, s, 1]]
    assert len(rose) == (0 if k_now == k + 1 else 1) and k_now in (k, k + 1), (rose, k, k_now)
    return (rose[0], -1) if rose else (k, int(cur["edges"][0, k, 2]))


def _follow(an, sp, rs, key, visit_limit, P, expl=None, want=lambda visits, k: True, stop=None, max_rounds=None):
    """Steps an analysis engine round by round and restates every root selection whose tree before
    it `want(root visits, root children)` selects.  Returns the counts: selections restated,
    selections where the rule without the root search picks otherwise, selections with a futile
    move, and the root children at each restated selection."""
    prev = None
    n = differ = with_futile = 0
    ks = []
    for _ in range(max_rounds or visit_limit + 8):
        an.step(1)
        head, _ = an.game_tree(0, 1)
        if len(head) == 0 or head[0, 0] == 0:
            continue
        visits, k = int(head[0, 0]), int(head[0, 10] & 0xFFFF)
        if visits >= visit_limit - 2 or (stop is not None and stop(n)):
            break  # before the visit limit: the slot still holds this tree
        if not want(visits, k):
            prev = None
            continue
        cur = _root_dump(an, 0, P)
        assert cur["nodes"][0, 0] == visits
        if prev is not None and visits == prev["nodes"][0, 0] + 1:
            slot, new_pos, nf = _root_select(prev, sp, rs, key, visit_limit, P, expl)
            assert (slot, new_pos) == _taken(prev, cur), (visits, slot, new_pos, _taken(prev, cur), nf)
            n += 1
            ks.append(int(prev["nodes"][0, 10] & 0xFFFF))
            with_futile += nf > 0
            differ += _root_select(prev, sp, {}, key, visit_limit, P, expl)[:2] != (slot, new_pos)
        prev = cur
    return n, differ, with_futile, ks


# ---------------------------------------------------------------------------------------
# 1. Off is off.

def test_off_is_off_and_late_setter_is_rejected(game_moves):
    q = [dict(id=5, moves=game_moves[:6])]

    def result(rs, expl):
        an, _ = _analysis(rs=rs, expl=expl, use_graph_search=1, root_num_symmetries_to_sample=2, **NOISE)
        h, m = _run(an, q)
        nodes, edges = an.game_tree(0, CAP)
        with pytest.raises(kc.CoffeeError, match="set_root_search"):
            an.set_root_search(**WIDE)
        an.close()
        return h.tobytes(), m.tobytes(), nodes.tobytes(), edges.tobytes()

    # never called, called with the defaults; then the same under the 8g mechanisms alone
    assert result(None, None) == result({}, None) == result(None, {})
    assert result(None, BOTH) == result({}, BOTH)
    assert result(None, None) != result(WIDE, None)
    an, _ = _analysis()
    an.step(1)
    rc = kc.lib().coffee_analysis_set_root_search(an.h, ctypes.byref(kc.default_root_search_params(**WIDE)))
    assert rc == -1  # COFFEE_EINVAL
    an.close()
    sp = kc.Selfplay(5, 5, 4, num_games=2, max_visits=8, node_cap=64)
    sp.set_root_search(**dict(WIDE, **FUTILE))
    with pytest.raises(kc.CoffeeError, match="wide_root_noise"):
        sp.set_root_search(wide_root_noise=5.5)
    with pytest.raises(kc.CoffeeError, match="futile_visits_threshold"):
        sp.set_root_search(futile_visits_threshold=0.001)
    sp.step(1)
    with pytest.raises(kc.CoffeeError, match="first round"):
        sp.set_root_search()
    sp.close()


# ---------------------------------------------------------------------------------------
# 2. The descent obeys the wide noise.

def test_descent_obeys_the_wide_noise(game_moves):
    P = 100
    query = dict(id=1, moves=game_moves[:2])
    an, sp = _analysis(rs=WIDE, **NOISE)
    an.submit([query])
    n, differ, _, _ = _follow(an, sp, WIDE, (SEED, 1, 0), VISITS, P)
    an.close()
    print("wide noise 0.5: %d root selections restated, %d where the noise-free rule chooses otherwise" % (n, differ))
    assert n >= 40
    assert differ >= 1  # otherwise the case does not tell the two rules apart
    # the draws are not the game stream's: the noised root policy and the stream's counter stay
    state = []
    for rs in (WIDE, None):
        an, _ = _analysis(rs=rs, **NOISE)
        _run(an, [query])
        state.append((an.root_policy(0).tobytes(), an.game_info(0)["rngCtr"], an.game_tree(0, CAP)[0].tobytes()))
        an.close()
    assert state[0][:2] == state[1][:2] and state[0][1] > 0
    assert state[0][2] != state[1][2]


# ---------------------------------------------------------------------------------------
# 3. The descent obeys the futile pruning, and the order futile -> funnel -> noise.

# (coefficient 0.25: the funnel then wants about one unit of weight of a 10 % move at 40 visits,
# so the leader keeps most of the weight and low-visit moves turn futile while the funnel asks
# for them)
# (wide noise at the reference's analysis value 0.04: at 0.5 the visits spread over so many moves
# that the leader's weight stays small and no move is futile within 64 visits)
ALL_ON = dict(rs=dict(FUTILE, wide_root_noise=0.04), expl=BOTH, over=dict(root_desired_per_child_visits_coeff=0.25))


@pytest.mark.parametrize("case", [dict(rs=FUTILE, expl=None, over={}), ALL_ON], ids=["futile", "all"])
def test_descent_obeys_the_futile_pruning(game_moves, case):
    P = 100
    an, sp = _analysis(rs=case["rs"], expl=case["expl"], **NOISE, **case["over"])
    an.submit([dict(id=1, moves=game_moves[:2])])
    n, differ, with_futile, _ = _follow(an, sp, case["rs"], (SEED, 1, 0), VISITS, P, expl=case["expl"])
    an.close()
    print("%s: %d root selections restated, %d with a futile move, %d where the plain rule chooses otherwise" %
          (case["rs"], n, with_futile, differ))
    assert n >= 40
    assert with_futile >= 1 and differ >= 1


# ---------------------------------------------------------------------------------------
# 4. Past 64 root children: selectBest<1> against selectBest<NI>.

WIDE_VISITS, WIDE_CAP = 380, 384


def test_root_selection_past_64_children():
    """7x7/5 with the cpuct of tests/test_gpu_exploration.py's wide-root case: the root's
    selections while it has at most 64 children (the one-item form) and past 64 (four items)."""
    X, Y, W, P = 7, 7, 5, 196
    rs = dict(WIDE, **FUTILE)
    an, sp = _analysis(X, Y, W, visits=WIDE_VISITS, cap=WIDE_CAP, rs=rs, cpuct_exploration=96.0,
                       root_desired_per_child_visits_coeff=4.0, **NOISE)
    an.submit([dict(id=1, moves=[])])
    # the first selections, and those from the 62nd child on (at most 40 of them)
    n, differ, with_futile, ks = _follow(an, sp, rs, (SEED, 1, 0), WIDE_VISITS, P,
                                         want=lambda visits, k: visits <= 24 or k >= 62,
                                         stop=lambda n: n >= 64, max_rounds=WIDE_VISITS + 8)
    an.close()
    small, large = sum(k <= 64 for k in ks), sum(k > 64 for k in ks)
    print("7x7: %d root selections restated (%d at <= 64 children, %d past 64, widest %d), %d with a futile move, "
          "%d where the plain rule chooses otherwise" % (n, small, large, max(ks), with_futile, differ))
    assert small >= 10 and large >= 5
    assert differ >= 1


# ---------------------------------------------------------------------------------------
# 5. Slot independence.

def test_a_query_does_not_depend_on_its_slot(game_moves):
    an, _ = _analysis(rs=dict(WIDE, **FUTILE), slots=4, **NOISE)
    same = dict(moves=game_moves[:2], stream=77, game_num=3)
    h, m = _run(an, [dict(id=1, **same), dict(id=2, moves=game_moves[:4]), dict(id=3, moves=[]), dict(id=4, **same)])
    trees = [an.game_tree(g, CAP) for g in range(4)]
    an.close()
    for name in h.dtype.names:
        if name != "id":
            assert h[0][name] == h[3][name], name
    assert m[0].tobytes() == m[3].tobytes() and h[0]["visits"] == VISITS
    assert m[0].tobytes() != m[1].tobytes()
    # the two searches ran in two slots and left the same tree in both
    twins = [(a, b) for a in range(4) for b in range(a + 1, 4)
             if len(trees[a][0]) > 1 and trees[a][0].tobytes() == trees[b][0].tobytes()
             and trees[a][1].tobytes() == trees[b][1].tobytes()]
    assert len(twins) == 1, twins


# ---------------------------------------------------------------------------------------
# 6. Fused against separate rounds.

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
    sp.set_root_search(**dict(WIDE, **FUTILE))
    return sp


@pytest.mark.parametrize("ci", [3, 16])
def test_fused_rounds_match_separate_rounds(ci):
    G = 32
    kw = dict(num_games=G, max_visits=48, seed=61, node_cap=CAP, commit_interval=ci, nn_cache_log2=10)
    a, b = _selfplay(True, **kw), _selfplay(False, **kw)
    a.enable_timing(1)
    b.enable_timing(1)
    done = 0
    # (to 2000 rounds: at commit interval 16 a 25-move game takes up to 25 * (48 + 16) rounds, and
    # the rows come with a game's end)
    for chunk in [5, 40, 700, 2000]:
        a.step(chunk - done)
        b.step(chunk - done)
        done = chunk
        for g in range(G):
            assert a.game_info(g) == b.game_info(g), (done, g)
            na, ea = a.game_tree(g, CAP)
            nb, eb = b.game_tree(g, CAP)
            np.testing.assert_array_equal(na, nb, err_msg="round %d game %d nodes" % (done, g))
            np.testing.assert_array_equal(ea, eb, err_msg="round %d game %d edges" % (done, g))
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
# 7. Match, per side.

def test_match_sides_carry_their_own_setting():
    X, Y, W, G, P = 5, 5, 4, 2, 100
    base = dict(max_visits=32, use_graph_search=0, root_num_symmetries_to_sample=1, root_noise_enabled=1, **PLAIN)
    sp = kc.default_match_params(**base)
    mt = kc.Match(X, Y, W, num_games=G, seed=SEED, node_cap=128, share_net=True, search=sp,
                  sides=(dict(base, **WIDE), dict(base)))
    with pytest.raises(kc.CoffeeError, match="side"):
        mt.set_root_search(side=-1, **WIDE)
    with pytest.raises(kc.CoffeeError, match="side"):
        mt.set_root_search(side=2, **WIDE)
    seen = {0: 0, 1: 0}
    differ = {0: 0, 1: 0}
    prev = [None] * G
    for _ in range(150):
        mt.step(1)
        for g in range(G):
            cur = _root_dump(mt, g, P)
            i = cur["info"]
            if i["phase"] != 1 or len(cur["nodes"]) == 0 or cur["nodes"][0, 0] == 0 or cur["nodes"][0, 0] >= 30:
                prev[g] = None
                continue
            pv = prev[g]
            prev[g] = cur
            if pv is None or (pv["info"]["gameNum"], pv["info"]["turn"]) != (i["gameNum"], i["turn"]) or \
                    cur["nodes"][0, 0] != pv["nodes"][0, 0] + 1:
                continue
            # the side that searches: the candidate (side 1) is black in game n of slot s iff s + n is even
            side = 1 if i["pla"] == (1 if (g + i["gameNum"]) % 2 == 0 else 2) else 0
            key = (SEED, g, i["gameNum"])
            noisy = _root_select(pv, sp, WIDE, key, 32, P)[:2]
            plain = _root_select(pv, sp, {}, key, 32, P)[:2]
            assert _taken(pv, cur) == (noisy if side == 0 else plain), (g, i, side, noisy, plain, _taken(pv, cur))
            seen[side] += 1
            differ[side] += noisy != plain
        if min(seen.values()) >= 12 and min(differ.values()) >= 1:
            break
    mt.close()
    print("root selections restated per side: %s, of them told apart by the noise: %s" % (seen, differ))
    # (told apart on both sides: side 1 followed the plain rule where the noisy one chose otherwise)
    assert min(seen.values()) >= 12 and min(differ.values()) >= 1
    # an engine without per-side settings takes -1 only
    mt = kc.Match(X, Y, W, num_games=G, seed=SEED, node_cap=128, search=kc.default_match_params(max_visits=8))
    for side in (0, 1):
        with pytest.raises(kc.CoffeeError, match="side"):
            mt.set_root_search(side=side, **WIDE)
    mt.set_root_search(**dict(WIDE, **FUTILE))
    mt.step(40)
    assert mt.stats()["errors"] == 0
    mt.close()


# ---------------------------------------------------------------------------------------
# 8. Commands.

def _move_name(pos):
    cell, d = pos % 25, pos // 25
    return chr(97 + cell % 5) + chr(97 + cell // 5) + chr(97 + d)


def test_analysis_command_reads_the_config_key(game_moves):
    moves = game_moves[:2]
    # the precondition: without the noise the search leaves legal moves unvisited here
    an = kc.Analysis(5, 5, 4, num_slots=2, seed=1, search=kc.default_analysis_params(max_visits=48))
    h, _ = an.analyze([dict(id=1, moves=moves)])
    legal = int((an.root_policy(0) >= 0).sum())
    an.close()
    assert int(h[0]["num_children"]) < legal
    cmd = [os.path.join(REPO, "katacoffee_amd", "katago"), "analysis", "-config",
           os.path.join(REPO, "configs", "analysis_coffee5.cfg"), "-override-config"]
    keys = "maxVisits=48,numAnalysisSlots=2,nnCacheSizePowerOfTwo=0"
    query = json.dumps(dict(id="a", moves=[_move_name(m) for m in moves])) + "\n"
    visited = []
    for extra in ("", ",wideRootNoise=0.5"):
        r = subprocess.run(cmd + [keys + extra], input=query, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip())
        assert out["rootInfo"]["visits"] == 48
        visited.append(sum(1 for i in out["moveInfos"] if i["visits"] > 0))
    print("root moves with visits: %d without, %d with wideRootNoise 0.5, %d legal" % (visited[0], visited[1], legal))
    assert visited[0] < legal
    assert visited[1] > visited[0]
    bad = subprocess.run(cmd + [keys + ",wideRootNoise=7"], input="", capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "wideRootNoise" in bad.stderr


def test_match_command_accepts_per_bot_keys(tmp_path):
    katago = os.path.join(REPO, "katacoffee_amd", "katago")
    model = str(tmp_path / "b2c32.cfnn")
    kc.write_random_model("b2c32", 0xBEEF, model)
    r = subprocess.run([katago, "match", "-config", os.path.join(REPO, "configs", "match_coffee5.cfg"),
                        "-sgf-output-dir", str(tmp_path / "sgf"), "-override-config",
                        "nnModelFile=%s,numGamesTotal=4,numGameThreads=4,maxVisits0=8,maxVisits1=8,seed=7,"
                        "nnCacheSizePowerOfTwo=10,nnPrecision=accurate,wideRootNoise0=0.5,"
                        "futileVisitsThreshold1=0.15" % model],
                       capture_output=True, text=True, timeout=120)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log
    assert "bot 0: wide root noise 0.5, futile visits threshold 0" in log, log
    assert "bot 1: wide root noise 0, futile visits threshold 0.15" in log, log
    bad = subprocess.run([katago, "match", "-config", os.path.join(REPO, "configs", "match_coffee5.cfg"),
                          "-sgf-output-dir", str(tmp_path / "sgf2"), "-override-config", "futileVisitsThreshold1=0"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "futileVisitsThreshold1" in (bad.stdout + bad.stderr)
