"""Parallel playouts per search on the device.  The frozen oracle makes one playout a
round, so a wide round is checked against a restatement made from the dumped trees: from the tree
before a round every descent of the round is recomputed in np.float32, in the kernel's operation
order -- the virtual losses of the round's earlier descents rebuilt from their paths, their
expansions applied, collisions included, kc.virtual_loss for the valuation (the kernels' own header
code on the host, pinned to float64 in tests/test_search_threads.py) -- and every level of every
path coffee_analysis_round_paths reports must be the one it names.  What the tree before the round
does not hold -- whether a node allocated in the round is terminal, and a non-root node's
expansion candidate after its first expansion of the round -- is read from the tree after it.
The round that reaches the visit limit has no tree after it (its report empties the slot): it is
restated from the tree before it alone -- the number of its descents, min(K, limit - visits),
every root selection and every level below that goes through nodes the tree before it describes;
a new node's kind is then the reported one, and the levels at a non-root node that was expanded
earlier in that round are taken as reported and counted.

5x5/4, the stand-in network, one analysis slot, 64 visits, node cap 256, no graph search, one
root symmetry and no NN cache unless stated."""
import numpy as np
import pytest

import katacoffee_amd as kc
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED, VISITS, CAP = 11, 64, 256
_f = np.float32
FLT_MAX = np.finfo(np.float32).max
PRUNE = dict(use_noise_pruning=1, noise_prune_utility_scale=0.15)
FACTOR = dict(cpuct_utility_stdev_scale=0.85, cpuct_utility_stdev_prior=0.40, cpuct_utility_stdev_prior_weight=2.0)
BOTH = dict(PRUNE, **FACTOR)  # the two mechanisms of DESIGN.md 8g
# root noise, without the root's move subtraction in the backup (the sums stay plain)
NOISE = dict(root_noise_enabled=1, chosen_move_subtract=0.0, chosen_move_prune=0.0)
# the restatement's own limits (it holds the kernel's sequence for these settings only)
PLAIN = dict(cpuct_exploration_log=0.0, fpu_parent_weight_by_visited_policy_pow=2.0)
# plain sums in the backup: a parent's sums are its children's (tests/test_gpu_exploration.py)
SUMS = dict(value_weight_exponent=0.0, subtree_value_bias_factor=0.0)
KEY = (SEED, 1, 0)  # the stream of query id 1: engine seed, stream, game number


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


def _analysis(X=5, Y=5, W=4, visits=VISITS, threads=1, per_thread=1.0, rs=None, expl=None, cap=CAP, slots=1,
              cache=0, **over):
    over.setdefault("use_graph_search", 0)
    over.setdefault("root_num_symmetries_to_sample", 1)
    params = kc.default_analysis_params(max_visits=visits, **dict(PLAIN, **over))
    an = kc.Analysis(X, Y, W, num_slots=slots, seed=SEED, node_cap=cap, nn_cache_log2=cache, query_capacity=32,
                     search=params)
    if expl is not None:
        an.set_exploration(**expl)
    if rs is not None:
        an.set_root_search(**rs)
    if threads is not None:
        an.set_search_threads(threads, per_thread)
    return an, params


def _dump(an, cap=CAP, slot=0):
    nodes, edges = an.game_tree(slot, cap)
    priors, next_prior, next_pos = an.game_tree_priors(slot, cap)
    assert len(priors) == len(nodes)
    return dict(nodes=nodes, edges=edges, priors=priors, next_prior=next_prior, next_pos=next_pos,
                root_policy=an.root_policy(slot), info=an.game_info(slot))


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


def _model(d, depth=None):
    """A dump as a dict keyed by the child-slot path from the root (no graph search: one per node):
    the node's record, its children (path, edge visits, move, prior) in slot order, its cached next
    expansion and its virtual losses (0: between rounds).  depth: only the nodes down to it."""
    nodes, edges = d["nodes"], d["edges"]
    pol = d["root_policy"]
    paths = {0: ()}
    M = {}
    for i in range(len(nodes)):
        if i not in paths:
            continue
        path = paths[i]
        k = int(nodes[i, 10] & 0xFFFF)
        rec = _f32(nodes[i, 1:8])  # ws, wsq, u, usq, wl, nnWin, nnLoss
        kids = []
        if depth is None or len(path) < depth:
            for j in range(k):
                c, mv = int(edges[i, j, 0]), int(edges[i, j, 2])
                assert 0 < c and c not in paths, "not a tree"
                paths[c] = path + (j,)
                prior = pol[mv] if i == 0 else d["priors"][i, j]
                kids.append(dict(path=path + (j,), ev=int(edges[i, j, 1]), move=mv, prior=_f(prior)))
        M[path] = dict(visits=int(nodes[i, 0]), ws=rec[0], u=rec[2], usq=rec[3], nn_win=rec[5], nn_loss=rec[6],
                       pla=int(nodes[i, 10] >> 16) & 0xFF, flags=int(nodes[i, 10] >> 24), kids=kids, vl=0,
                       nxt=(_f(d["next_prior"][i]), int(d["next_pos"][i])) if "next_pos" in d else None)
    return M


def _select(M, path, sp, rs, expl, per_thread, visit_limit, turn, P, pol, use_vl=True):
    """selectBest (search.hip; selectBestChildToDescend searchexplorehelpers.cpp:304-451) at a node
    of the model in np.float32, in the kernel's operation order: the virtual-loss valuation after
    the choice between the first-play urgency and the child's utility, before futile-visit pruning,
    the desired-per-child funnel and the wide root noise.  Returns (slot, new move or -1);
    slot == number of children: a new child; -1: none selectable."""
    n = M[path]
    is_root = path == ()
    wide = float(rs.get("wide_root_noise", 0.0)) if is_root else 0.0
    thr = float(rs.get("futile_visits_threshold", 0.0)) if is_root else 0.0
    kids = n["kids"]
    k, pla, visits = len(kids), n["pla"], n["visits"]
    p = [c["prior"] for c in kids]
    ch = [M[c["path"]] for c in kids]
    probs = [_f(0) if p[j] < 0 else p[j] for j in range(k)]
    cw = [_f(0) if p[j] < 0 else _child_weight(kids[j]["ev"], ch[j]["visits"], ch[j]["ws"]) for j in range(k)]
    prob_mass, total = _tree_sum64(probs), _tree_sum64(cw)
    # fpuValue
    parent_u = n["u"]
    for_fpu = parent_u
    if sp.fpu_parent_weight_by_visited_policy:
        assert sp.fpu_parent_weight_by_visited_policy_pow == 2.0
        avg_w = min(_f(1), _f(prob_mass * prob_mass))
        for_fpu = _f(_f(avg_w * parent_u) + _f(_f(_f(1) - avg_w) * _f(n["nn_win"] - n["nn_loss"])))
    red_max = _f(sp.root_fpu_reduction_max if is_root else sp.fpu_reduction_max)
    loss_prop = _f(sp.root_fpu_loss_prop if is_root else sp.fpu_loss_prop)
    reduction = _f(red_max * np.sqrt(prob_mass))
    fpu = _f(for_fpu - reduction) if pla == 2 else _f(for_fpu + reduction)
    loss_value = _f(-1) if pla == 2 else _f(1)
    fpu = _f(fpu + _f(_f(loss_value - fpu) * loss_prop))
    # exploreScaling and the stdev factor
    assert sp.cpuct_exploration_log == 0.0
    scaling = _f(_f(sp.cpuct_exploration) * np.sqrt(_f(total + _f(0.01))))
    if expl is not None:
        scaling = _f(scaling * _stdev_factor(visits, n["ws"], n["u"], n["usq"], expl["cpuct_utility_stdev_prior"],
                                             expl["cpuct_utility_stdev_prior_weight"],
                                             expl["cpuct_utility_stdev_scale"]))
    max_w = max([_f(0)] + cw)
    left = visit_limit - visits

    def noised(u, prior, pos):
        if not wide > 0:
            return u, prior
        sm, bonus = kc.wide_root_noise(KEY[0], KEY[1], KEY[2], turn, visits, pos, prior, wide_root_noise=wide)
        return (_f(u + bonus) if pla == 2 else _f(u - bonus)), sm

    best, best_slot = -np.inf, -1
    coeff = _f(sp.root_desired_per_child_visits_coeff)
    for j in range(k):
        if p[j] < 0:
            continue
        w = cw[j]
        u = fpu if (ch[j]["visits"] == 0 or w <= 0) else ch[j]["u"]
        if use_vl and ch[j]["vl"] > 0:
            u, w = kc.virtual_loss(per_thread, ch[j]["vl"], pla, u, w)
        if thr > 0 and kc.futile_visits(max_w, n["ws"], visits, left, kids[j]["ev"], ch[j]["visits"], w,
                                        futile_visits_threshold=thr):
            val = -FLT_MAX
        elif is_root and coeff > 0 and p[j] > 0 and w < np.sqrt(_f(_f(p[j] * total) * coeff)):
            val = _f(1e20)
        else:
            u, pj = noised(u, p[j], kids[j]["move"])
            val = _f(_f(_f(scaling * pj) / _f(_f(1) + w)) + (u if pla == 2 else -u))
        if val > best:
            best, best_slot = val, j
    bp, bpos = _f(-1), -1
    if is_root:
        has = np.zeros(P, bool)
        has[[c["move"] for c in kids]] = True
        for pos in range(P):
            if not has[pos] and pol[pos] >= 0 and pol[pos] > bp:
                bp, bpos = pol[pos], pos
    elif n["nxt"][1] != 0xFFFF:
        bp, bpos = n["nxt"]
    new_pos = -1
    if bpos >= 0:
        if thr > 0 and kc.futile_visits(max_w, n["ws"], visits, left, is_new=True, futile_visits_threshold=thr):
            val = -FLT_MAX
        else:
            u, bp2 = noised(fpu, bp, bpos)
            val = _f(_f(_f(scaling * bp2) / _f(1)) + (u if pla == 2 else -u))
        if val > best:
            best_slot, new_pos = k, bpos
    return best_slot, new_pos


def _new_node(terminal):
    return dict(visits=0, ws=_f(0), u=_f(0), usq=_f(0), nn_win=_f(0), nn_loss=_f(0), pla=0,
                flags=2 if terminal else 0, kids=[], vl=1, nxt=(_f(-1), 0xFFFF))


def _take_reported(M, path, rep, level):
    """The rest of a reported path from `level` on, applied to the model unchecked: the virtual
    losses it leaves, and a node it allocates (whose parent's next candidate is then unknown)."""
    for slot in rep["child_slots"][level:]:
        n = M[path]
        if slot < len(n["kids"]):
            path = n["kids"][slot]["path"]
            M[path]["vl"] += 1
        else:
            assert slot == len(n["kids"])
            path = path + (slot,)
            n["kids"].append(dict(path=path, ev=0, move=-1, prior=None))
            n["nxt"] = None
            M[path] = _new_node(rep["leaf_kind"] == kc.LEAF_TERMINAL)


def _restate_round(pre, post, reported, K, sp, rs, expl, per_thread, visit_limit, P, full):
    """The descents of one round from the tree before it; every level (full) or the root level of
    every reported path must be the restated one, and so must its leaf kind.  post None (the
    search's last round): see the module's docstring.  Returns the counts: levels compared,
    levels where the rule without virtual losses chooses otherwise, collisions, levels taken as
    reported in a last round."""
    depth = None if full else 1
    M, after = _model(pre, depth), (_model(post, depth) if post is not None else None)
    pol, turn = pre["root_policy"], pre["info"]["turn"]
    want = min(K, visit_limit - M[()]["visits"])
    assert 1 <= len(reported) <= want
    levels = differ = collisions = taken = 0
    for j, rep in enumerate(reported):
        path, slots, kind, hit = (), [], None, None
        while kind is None:
            n = M[path]
            if n["flags"] & 2:
                kind = kc.LEAF_TERMINAL
                break
            if (not full and path != ()) or n["nxt"] is None:
                # root level only: the rest of the path as reported (it bears no virtual loss the
                # root's selection could see).  Likewise, in a last round, from a non-root node
                # whose next candidate the tree before the round does not tell.
                assert rep["child_slots"][:len(slots)] == slots
                if full:
                    taken += len(rep["child_slots"]) - len(slots) + (rep["collision"] is not None)
                    _take_reported(M, path, rep, len(slots))
                slots, kind = list(rep["child_slots"]), rep["leaf_kind"]
                hit = None if rep["collision"] is None else rep["collision"][1]
                break
            slot, new_pos = _select(M, path, sp, rs, expl, per_thread, visit_limit, turn, P, pol)
            plain = _select(M, path, sp, rs, expl, per_thread, visit_limit, turn, P, pol, use_vl=False)
            levels += 1
            differ += plain != (slot, new_pos)
            k = len(n["kids"])
            if slot < 0:
                kind = kc.LEAF_NOCHILD
            elif slot == k:
                cpath = path + (k,)
                if after is not None:
                    assert after[cpath]["kids"] == [] or not full
                    terminal = after[cpath]["flags"] & 2
                else:
                    terminal = rep["leaf_kind"] == kc.LEAF_TERMINAL
                prior = pol[new_pos] if path == () else n["nxt"][0]
                n["kids"].append(dict(path=cpath, ev=0, move=new_pos, prior=_f(prior)))
                M[cpath] = _new_node(terminal)
                if path != () and after is None:
                    n["nxt"] = None  # unknown from here on
                elif path != ():  # the node's following candidate: its next child of the tree after, or its cache
                    a = after[path]
                    assert a["kids"][k]["move"] == new_pos and a["kids"][k]["prior"] == _f(prior)
                    n["nxt"] = (a["kids"][k + 1]["prior"], a["kids"][k + 1]["move"]) if len(a["kids"]) > k + 1 else a["nxt"]
                slots.append(slot)
                kind = kc.LEAF_TERMINAL if terminal else kc.LEAF_NN
            else:
                c = M[n["kids"][slot]["path"]]
                if c["flags"] & 3 == 0:
                    kind, hit = kc.LEAF_COLLISION, slot
                else:
                    assert n["kids"][slot]["ev"] == c["visits"]  # (no graph search: never a catch-up)
                    c["vl"] += 1
                    slots.append(slot)
                    path = n["kids"][slot]["path"]
        got = (list(rep["child_slots"]), rep["leaf_kind"], None if rep["collision"] is None else rep["collision"][1])
        assert got == (slots, kind, hit), (j, got, slots, kind, hit)
        if kind == kc.LEAF_COLLISION:
            collisions += 1
            assert j == len(reported) - 1  # the slot makes no further descent that round
    assert collisions == 1 or len(reported) == want
    return levels, differ, collisions, taken


def _check_sums(d):
    """Every parent's sums against their float64 recomputation from its children (value weighting,
    SVB, graph search and uncertainty off: a child weighs its own weight sum, the node's own
    evaluation 1): relative 1e-5 with the cancellation rule of tests/test_gpu_exploration.py.
    Also edge visits == child visits and visits == 1 + sum of edge visits.  Returns the largest
    relative difference."""
    nodes, edges = d["nodes"], d["edges"]
    worst = 0.0
    for i in range(len(nodes)):
        rec = _f32(nodes[i, 1:8]).astype(np.float64)
        flags, k = int(nodes[i, 10] >> 24), int(nodes[i, 10] & 0xFFFF)
        assert flags & 3, "a node left in flight"
        if flags & 2:
            assert k == 0
            continue
        self_u = rec[5] - rec[6]
        ci = edges[i, :k, 0].astype(np.int64)
        kids = _f32(nodes[ci, 1:6]).astype(np.float64).reshape(k, 5)
        np.testing.assert_array_equal(edges[i, :k, 1], nodes[ci, 0])
        assert nodes[i, 0] == 1 + edges[i, :k, 1].sum()
        good = (nodes[ci, 0] > 0) & (kids[:, 0] > 0)
        assert good.all()
        w = kids[:, 0]
        ws = w.sum() + 1.0
        want = [ws, kids[:, 1].sum() + 1.0, ((w * kids[:, 2]).sum() + self_u) / ws,
                ((w * kids[:, 3]).sum() + self_u * self_u) / ws, ((w * kids[:, 4]).sum() + self_u) / ws]
        scale = [ws, want[1], ((w * np.abs(kids[:, 2])).sum() + abs(self_u)) / ws, want[3],
                 ((w * np.abs(kids[:, 4])).sum() + abs(self_u)) / ws]
        for name, got, wnt, sc in zip(["weightSum", "weightSqSum", "utilityAvg", "utilitySqAvg", "winLossAvg"],
                                      rec[:5], want, scale):
            if abs(wnt) >= 0.1 * sc:
                rel = abs(got - wnt) / abs(wnt)
                worst = max(worst, rel)
                assert rel <= 1e-5, (i, k, name, got, wnt)
            else:
                assert abs(got - wnt) <= 1e-5 * sc, (i, k, name, got, wnt, sc)
    return worst


def _follow(an, sp, K, visit_limit, P, rs=None, expl=None, per_thread=1.0, full=False, cap=CAP, sums=True,
            want=lambda visits, k: True, stop=None):
    """Steps an engine that holds one query round by round and restates every search round, the
    one that reaches the visit limit from the tree before it alone; returns after that round (or
    at `stop`).  After every round: no live virtual loss, the parents' sums (sums) and the visit
    counts.  Returns the summed counts of _restate_round (without the last), the rounds restated,
    the largest relative difference of the sums and the root's children at each restated round."""
    tot = np.zeros(4, np.int64)
    rounds, worst, ks = 0, 0.0, []
    for _ in range(visit_limit + 8):
        info = an.game_info(0)
        head, _ = an.game_tree(0, 1)
        searching = info["phase"] == 1 and len(head) == 1 and head[0, 0] > 0
        visits = int(head[0, 0]) if searching else 0
        k = int(head[0, 10] & 0xFFFF) if searching else 0
        if stop is not None and stop(rounds):
            break
        restate = searching and want(visits, k)
        pre = _dump(an, cap if full else P + 1) if restate else None
        an.step(1)
        assert an.search_threads_info()["live_virtual_losses"] == 0
        if not searching:
            assert an.round_paths(0) == []
            continue
        reported = an.round_paths(0)
        made = sum(r["leaf_kind"] != kc.LEAF_COLLISION for r in reported)  # a root visit each
        if visits + made >= visit_limit:
            # the search's last round: the slot is reported and emptied, the paths remain
            assert visits + made == visit_limit and an.game_info(0)["phase"] != 1
            if restate:
                n = _restate_round(pre, None, reported, K, sp, rs or {}, expl, per_thread, visit_limit, P, full)
                print("last round: %d descents of min(K, limit - visits) = %d, %d levels restated, %d taken as "
                      "reported" % (len(reported), min(K, visit_limit - visits), n[0], n[3]))
                tot[:3] += n[:3]
                rounds += 1
            break
        assert an.game_tree(0, 1)[0][0, 0] == visits + made
        post = _dump(an, cap) if restate or sums else None
        if sums:
            worst = max(worst, _check_sums(post))
        if restate:
            tot += _restate_round(pre, post, reported, K, sp, rs or {}, expl, per_thread, visit_limit, P, full)
            rounds += 1
            ks.append(k)
    return tot[:3], rounds, worst, ks


def _finish(an, visit_limit):
    """Steps to the query's result; it reports exactly the visit limit."""
    for _ in range(visit_limit + 8):
        an.step(1)
        h, m = an.drain()
        if len(h):
            assert an.stats()["errors"] == 0 and h[0]["status"] == kc.ANALYSIS_OK
            assert h[0]["visits"] == visit_limit
            assert m[0]["edge_visits"][:h[0]["num_children"]].sum() == visit_limit - 1
            assert an.search_threads_info()["live_virtual_losses"] == 0
            return h, m
    raise AssertionError("the query did not finish")


# ---------------------------------------------------------------------------------------
# 1. Restated descents.

def test_every_level_of_every_path_k4(game_moves):
    P = 100
    an, sp = _analysis(threads=4, **SUMS)
    an.submit([dict(id=1, moves=game_moves[:2])])
    (levels, differ, collisions), rounds, worst, _ = _follow(an, sp, 4, VISITS, P, full=True)
    _finish(an, VISITS)
    info = an.search_threads_info()
    an.close()
    print("K = 4: %d rounds, %d levels restated, %d where the K = 1 rule chooses otherwise, %d collisions; "
          "sums: largest relative difference %.3e" % (rounds, levels, differ, collisions, worst))
    assert rounds >= 12 and levels >= 80
    assert differ >= 1  # otherwise the case shows nothing
    assert info["threads"] == 4 and info["descents"] >= VISITS - 1 and info["collisions"] >= collisions


ROOT_CASES = {
    "k8": dict(threads=8),
    "wide": dict(threads=4, rs=dict(wide_root_noise=0.04), over=NOISE),
    "futile": dict(threads=4, rs=dict(futile_visits_threshold=0.4), over=NOISE),
    "expl": dict(threads=4, expl=BOTH, over=NOISE, sums=False),
}


@pytest.mark.parametrize("name", list(ROOT_CASES))
def test_root_level_of_every_path(game_moves, name):
    P = 100
    case = ROOT_CASES[name]
    K = case["threads"]
    an, sp = _analysis(threads=K, rs=case.get("rs"), expl=case.get("expl"), **SUMS, **case.get("over", {}))
    an.submit([dict(id=1, moves=game_moves[:2])])
    (levels, differ, collisions), rounds, worst, _ = _follow(an, sp, K, VISITS, P, rs=case.get("rs"),
                                                             expl=case.get("expl"), sums=case.get("sums", True))
    _finish(an, VISITS)
    an.close()
    print("%s: %d rounds, %d root selections restated, %d where the K = 1 rule chooses otherwise, %d collisions; "
          "sums: largest relative difference %.3e" % (name, rounds, levels, differ, collisions, worst))
    assert levels >= 40
    assert differ >= 1


WIDE_VISITS, WIDE_CAP = 380, 384


def test_root_level_past_64_children():
    """7x7/5 with the settings of tests/test_gpu_root_search.py's wide-root case: the root's
    selections while it has at most 64 children (the one-item form) and past 64 (four items)."""
    X, Y, W, P = 7, 7, 5, 196
    an, sp = _analysis(X, Y, W, visits=WIDE_VISITS, cap=WIDE_CAP, threads=4, cpuct_exploration=96.0,
                       root_desired_per_child_visits_coeff=4.0, **SUMS, **NOISE)
    an.submit([dict(id=1, moves=[])])
    (levels, differ, collisions), rounds, worst, ks = _follow(
        an, sp, 4, WIDE_VISITS, P, cap=WIDE_CAP, sums=False, want=lambda visits, k: visits <= 8 or k >= 63,
        stop=lambda n: n >= 26)
    an.close()
    small, large = sum(k <= 64 for k in ks), sum(k > 64 for k in ks)
    print("7x7: %d rounds restated (%d at <= 64 root children, %d past 64, widest %d), %d root selections, "
          "%d where the K = 1 rule chooses otherwise" % (rounds, small, large, max(ks), levels, differ))
    assert small >= 3 and large >= 4
    assert differ >= 1


# ---------------------------------------------------------------------------------------
# 2. Visit limits K does not divide, and collisions.

def test_exact_visits_with_a_limit_k_does_not_divide(game_moves):
    an, sp = _analysis(visits=50, threads=8, **SUMS)
    an.submit([dict(id=1, moves=game_moves[:4])])
    (levels, differ, collisions), rounds, worst, _ = _follow(an, sp, 8, 50, 100)
    _finish(an, 50)
    an.close()
    assert rounds >= 4 and worst <= 1e-5


# The position after the line's first six moves, chosen on the GPU among the line's prefixes of 0
# to 12 moves: its root has three children at the end and a round's eight descents meet in the
# same nodes -- 3 collisions in 18 descents, the most of the thirteen (six of them show none).
COLLISION_PREFIX = 6


def test_collisions_happen_and_are_handled(game_moves):
    an, sp = _analysis(visits=16, threads=8, **SUMS)
    an.submit([dict(id=1, moves=game_moves[:COLLISION_PREFIX])])
    (levels, differ, collisions), rounds, worst, _ = _follow(an, sp, 8, 16, 100, full=True)
    _finish(an, 16)
    info = an.search_threads_info()
    an.close()
    print("K = 8, 16 visits: %d descents, %d collisions (%d in the %d restated rounds)" %
          (info["descents"], info["collisions"], collisions, rounds))
    assert info["collisions"] > 0
    assert collisions > 0  # and restated


# ---------------------------------------------------------------------------------------
# 3. Off is off; slot independence.

@pytest.fixture(scope="module")
def two_games():
    """The two lines of tests/test_gpu_analysis.py's slot-independence case."""
    out = []
    for seed in (SEED, SEED + 1):
        ora = oracle.Selfplay(5, 5, 4, games=1, max_visits=24, node_cap=128, seed=seed, slot_base=3)
        moves = []
        while len(moves) < 10:
            ora.rounds(1)
            i = ora.info(0)
            if i["movesMade"] > len(moves):
                assert i["gameNum"] == 0 and i["lastCell"] >= 0, i
                moves.append(i["lastDir"] * 25 + i["lastCell"])
        out.append(moves)
    return out


def test_off_is_off(two_games):
    """The 19-query set of tests/test_gpu_analysis.py's slot-independence case through four slots:
    an engine set to one thread against one never set."""
    qs = [dict(id=1000 + i, moves=two_games[i % 2][:i // 2], max_visits=[8, 24, 40][i % 3]) for i in range(19)]

    def result(threads):
        params = kc.default_analysis_params(max_visits=VISITS)
        an = kc.Analysis(5, 5, 4, num_slots=4, seed=SEED, node_cap=CAP, query_capacity=32, search=params)
        if threads is not None:
            an.set_search_threads(threads, 1.0)
        h, m = an.analyze(qs, rounds_per_step=7)
        # (which slot takes which query is the scheduler's: the slots' last trees as a set)
        trees = sorted(t[0].tobytes() + t[1].tobytes() for t in (an.game_tree(g, CAP) for g in range(4)))
        assert an.stats()["errors"] == 0
        an.close()
        return h.tobytes(), m.tobytes(), trees

    never, one, four = result(None), result(1), result(4)
    assert never[0] == one[0], "headers"
    assert never[1] == one[1], "move records"
    assert never[2] == one[2], "trees"
    assert never[0] != four[0] and never[1] != four[1]


def test_a_query_does_not_depend_on_its_slot(game_moves):
    qs = [dict(id=1 + i, moves=game_moves[:2 * i], stream=40 + i) for i in range(6)]
    an, _ = _analysis(visits=40, threads=4, slots=2, cache=10)
    h2, m2 = an.analyze(qs)
    an.close()
    assert np.all(h2["visits"] == 40)
    for i, q in enumerate(qs):
        an, _ = _analysis(visits=40, threads=4, slots=1, cache=10)
        h1, m1 = an.analyze([q])
        an.close()
        assert h1[0].tobytes() == h2[i].tobytes() and m1[0].tobytes() == m2[i].tobytes(), i


# ---------------------------------------------------------------------------------------
# 4. Refusals.

def test_refusals_leave_the_engine_usable(game_moves):
    an, _ = _analysis(visits=16, threads=None, slots=4)
    for bad in (0, 33):
        with pytest.raises(kc.CoffeeError, match="threads must be in 1..32"):
            an.set_search_threads(bad)
    with pytest.raises(kc.CoffeeError, match="virtual_losses_per_thread"):
        an.set_search_threads(4, 0.0)
    assert kc.lib().coffee_analysis_set_search_threads(an.h, 0, 1.0) == -1  # COFFEE_EINVAL
    assert an.search_threads_info()["threads"] == 1
    an.submit([dict(id=1, moves=game_moves[:2])])
    an.step(2)
    with pytest.raises(kc.CoffeeError, match="holds no query"):
        an.set_search_threads(4)
    for _ in range(40):
        an.step(1)
        h, _m = an.drain()
        if len(h):
            break
    assert len(h) == 1 and h[0]["visits"] == 16
    # between queries the setting may change
    an.set_search_threads(4, 2.0)
    info = an.search_threads_info()
    assert info["threads"] == 4 and info["virtual_losses_per_thread"] == 2.0
    h, _m = an.analyze([dict(id=2, moves=game_moves[:2])])
    assert h[0]["visits"] == 16 and an.stats()["errors"] == 0
    an.close()
    # a round must fit one network launch: 4 slots x 4 threads past a batch cap of 8
    params = kc.default_analysis_params(max_visits=16)
    an = kc.Analysis(5, 5, 4, num_slots=4, seed=SEED, node_cap=64, nn_batch_cap=8, search=params)
    with pytest.raises(kc.CoffeeError, match="batch cap"):
        an.set_search_threads(4)
    an.set_search_threads(2)
    h, _m = an.analyze([dict(id=3, moves=game_moves[:2])])
    assert h[0]["visits"] == 16 and an.stats()["errors"] == 0
    an.close()
    with pytest.raises(kc.CoffeeError, match="batch cap"):
        kc.Analysis(5, 5, 4, num_slots=4, seed=SEED, node_cap=64, nn_batch_cap=8, search=params, search_threads=4)


# ---------------------------------------------------------------------------------------
# 5. 9x9/5: the seven-item kernels.

def test_9x9_runs_the_seven_item_kernels():
    an, sp = _analysis(9, 9, 5, visits=24, threads=2, cap=64, **SUMS)
    an.submit([dict(id=1, moves=[])])
    (levels, differ, collisions), rounds, worst, _ = _follow(an, sp, 2, 24, 324, cap=64)
    _finish(an, 24)
    an.close()
    print("9x9: %d rounds, %d root selections restated, sums: largest relative difference %.3e" %
          (rounds, levels, worst))
    assert rounds >= 8
