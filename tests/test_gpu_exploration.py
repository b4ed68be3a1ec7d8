"""Variance-scaled exploration and noise pruning on the device.  The frozen oracle
knows neither rule, so with them on the device is checked against restatements made from the
dumped trees: every parent's sums are the sums of its children's records under the float64
slot-order pruning scan, every level of every playout takes the child the np.float32 selection
rule with the stdev factor picks, and the reported play-selection values follow the scaled
exploration.  Off, nothing changes.

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
PRUNE = dict(use_noise_pruning=1, noise_prune_utility_scale=0.15)
FACTOR = dict(cpuct_utility_stdev_scale=0.85, cpuct_utility_stdev_prior=0.40, cpuct_utility_stdev_prior_weight=2.0)
BOTH = dict(PRUNE, **FACTOR)
NOISE = dict(root_noise_enabled=1)


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


def _analysis(X=5, Y=5, W=4, visits=VISITS, expl=None, cap=CAP, **over):
    over.setdefault("use_graph_search", 0)
    over.setdefault("root_num_symmetries_to_sample", 1)
    params = kc.default_analysis_params(max_visits=visits, **over)
    an = kc.Analysis(X, Y, W, num_slots=1, seed=SEED, node_cap=cap, nn_cache_log2=0, query_capacity=8, search=params)
    if expl is not None:
        an.set_exploration(**expl)
    return an, params


def _run(an, queries):
    h, m = an.analyze(queries)
    st = an.stats()
    assert st["errors"] == 0 and np.all(h["status"] == kc.ANALYSIS_OK)
    return h, m


def _paths(nodes, edges):
    """The move path from the root to every node of a dumped tree (no graph search: one each)."""
    paths = {0: []}
    for i in range(len(nodes)):
        for j in range(int(nodes[i, 10] & 0xFFFF)):
            c, mv = int(edges[i, j, 0]), int(edges[i, j, 2])
            assert 0 < c < len(nodes) and c not in paths, "not a tree"
            paths[c] = paths[i] + [mv]
    assert len(paths) == len(nodes)
    return [tuple(paths[i]) for i in range(len(nodes))]


def _dump(an, cap=CAP):
    nodes, edges = an.game_tree(0, cap)
    priors, next_prior, next_pos = an.game_tree_priors(0, cap)
    assert len(priors) == len(nodes)
    return dict(nodes=nodes, edges=edges, priors=priors, next_prior=next_prior, next_pos=next_pos,
                root_policy=an.root_policy(0))


# ---------------------------------------------------------------------------------------
# 4. Off is off.

def test_off_is_off_and_late_setter_is_rejected(game_moves):
    q = [dict(id=5, moves=game_moves[:6])]
    out = []
    for expl in (None, {}, dict(noise_prune_utility_scale=0.3, cpuct_utility_stdev_prior=0.7, noise_pruning_cap=2.0)):
        an, _ = _analysis(expl=expl, use_graph_search=1, root_num_symmetries_to_sample=2, **NOISE)
        h, m = _run(an, q)
        nodes, edges = an.game_tree(0, CAP)
        out.append((h.tobytes(), m.tobytes(), nodes.tobytes(), edges.tobytes()))
        with pytest.raises(kc.CoffeeError, match="set_exploration"):
            an.set_exploration(**BOTH)
        an.close()
    assert out[0] == out[1] == out[2]
    an, _ = _analysis()
    an.step(1)
    rc = kc.lib().coffee_analysis_set_exploration(an.h, ctypes.byref(kc.default_exploration_params(**BOTH)))
    assert rc == -1  # COFFEE_EINVAL
    an.close()
    sp = kc.Selfplay(5, 5, 4, num_games=2, max_visits=8, node_cap=64)
    sp.set_exploration(**BOTH)
    with pytest.raises(kc.CoffeeError, match="cpuct_utility_stdev_scale"):
        sp.set_exploration(cpuct_utility_stdev_scale=2.0)
    sp.step(1)
    with pytest.raises(kc.CoffeeError, match="first round"):
        sp.set_exploration()
    sp.close()


def test_on_and_off_differ(game_moves):
    # (two moves in: deeper into this line the play is forced and 64 visits leave nothing to prune)
    q = [dict(id=1, moves=game_moves[:2])]
    trees = []
    for expl in ({}, BOTH, PRUNE, FACTOR):
        an, _ = _analysis(expl=expl, **NOISE)
        _run(an, q)
        trees.append(an.game_tree(0, CAP))
        an.close()
    (n0, e0) = trees[0]
    for n1, e1 in trees[1:]:
        assert n0.shape != n1.shape or not np.array_equal(n0, n1) or not np.array_equal(e0, e1)


# ---------------------------------------------------------------------------------------
# 5. The recompute obeys the pruning.

CANCEL_FLOOR = 0.1


def _prune64(w, u, p, utility_scale, cap=np.inf):
    """pruneNoiseWeight (searchupdatehelpers.cpp:423-467) in float64 over the good children in
    slot order; returns the new weights and the scan's total."""
    total = float(np.sum(w))
    if len(w) <= 1 or total <= 0.00001:
        return np.array(w, np.float64), total
    usum = wsum = psum = 0.0
    out = []
    for old, ui, pi in zip(w, u, p):
        pi = max(1e-30, pi)
        nw = old
        if wsum > 0 and psum > 0:
            gap = usum / wsum - ui
            if gap > 0:
                lenient = 2.0 * (wsum * pi / psum)
                if old > lenient:
                    nw = old - min((old - lenient) * (1.0 - np.exp(-gap / utility_scale)), cap)
        usum += ui * nw
        wsum += nw
        psum += pi
        out.append(nw)
    return np.array(out, np.float64), wsum


def _check_pruned_sums(d, utility_scale, prune=True):
    """recomputeNodeStats in float64 from the dump with noise pruning (value weighting and SVB
    off, no graph search, uncertainty off: a child's weight before pruning is its own weight sum
    and the node's own evaluation weighs 1).  Plain relative 1e-5 on all five sums with the
    cancellation rule of tests/test_gpu_uncertainty.py::_check_sums: the same sums with at most
    one more rounding per term.  Returns the number of parents, the number of parents whose
    weightSum lies below the plain sum by more than 1e-3 relative, and the largest relative
    difference over the values held to the plain bound."""
    nodes, edges, priors = d["nodes"], d["edges"], d["priors"]
    worst = 0.0
    parents = pruned = 0
    for i in range(len(nodes)):
        rec = _f32(nodes[i, 1:8]).astype(np.float64)  # ws, wsq, u, usq, wl, nnWin, nnLoss
        flags, k = int(nodes[i, 10] >> 24), int(nodes[i, 10] & 0xFFFF)
        next_pla = int(nodes[i, 10] >> 16) & 0xFF
        if flags & 2 or not flags & 1:
            assert k == 0
            continue
        assert nodes[i, 21] == 0  # uncertainty weighting off
        self_u = rec[5] - rec[6]
        ci = edges[i, :k, 0].astype(np.int64)
        kids = _f32(nodes[ci, 1:6]).astype(np.float64).reshape(k, 5)
        np.testing.assert_array_equal(edges[i, :k, 1], nodes[ci, 0])
        assert nodes[i, 0] == 1 + edges[i, :k, 1].sum()
        good = (nodes[ci, 0] > 0) & (kids[:, 0] > 0)
        kids = kids[good]
        pr = (d["root_policy"][edges[i, :k, 2].astype(np.int64)] if i == 0 else priors[i, :k]).astype(np.float64)[good]
        plain = kids[:, 0]
        if prune:
            self_util = kids[:, 2] if next_pla == 2 else -kids[:, 2]
            w, total = _prune64(plain, self_util, pr, float(_f(utility_scale)))
        else:
            w, total = plain, plain.sum()
        ws = total + 1.0
        want = [ws, (((w / kids[:, 0]) ** 2) * kids[:, 1]).sum() + 1.0,
                ((w * kids[:, 2]).sum() + self_u) / ws,
                ((w * kids[:, 3]).sum() + self_u * self_u) / ws,
                ((w * kids[:, 4]).sum() + self_u) / ws]
        scale = [ws, want[1], ((w * np.abs(kids[:, 2])).sum() + abs(self_u)) / ws, want[3],
                 ((w * np.abs(kids[:, 4])).sum() + abs(self_u)) / ws]
        for name, got, wnt, sc in zip(["weightSum", "weightSqSum", "utilityAvg", "utilitySqAvg", "winLossAvg"],
                                      rec[:5], want, scale):
            rel = abs(got - wnt) / abs(wnt) if wnt != 0.0 else float(got != 0.0)
            if abs(wnt) >= CANCEL_FLOOR * sc:
                worst = max(worst, rel)
                assert rel <= 1e-5, (i, k, name, got, wnt)
            else:
                assert abs(got - wnt) <= 1e-5 * sc, (i, k, name, got, wnt, sc)
        parents += k > 0
        pruned += k > 0 and rec[0] < (plain.sum() + 1.0) * (1.0 - 1e-3)
    return parents, pruned, worst


SUMS = dict(value_weight_exponent=0.0, subtree_value_bias_factor=0.0)


def test_recompute_obeys_the_pruning(game_moves):
    an, _ = _analysis(expl=PRUNE, **SUMS, **NOISE)
    _run(an, [dict(id=1, moves=game_moves[:2])])
    d = _dump(an)
    an.close()
    assert d["nodes"][0, 0] == VISITS
    parents, pruned, worst = _check_pruned_sums(d, 0.15)
    print("64-visit line: %d parents, %d pruned by more than 1e-3, largest relative difference %.3e" %
          (parents, pruned, worst))
    assert parents >= 10
    # without this the case proves nothing (and without the feature no weight sum is lowered)
    assert pruned >= 1


def test_recompute_obeys_the_pruning_wide_root():
    """48 visits on the empty board: the root reads its edge-pool block (more than 16 children)."""
    an, _ = _analysis(visits=48, expl=PRUNE, **SUMS, **NOISE)
    _run(an, [dict(id=1, moves=[])])
    d = _dump(an)
    an.close()
    k = int(d["nodes"][0, 10] & 0xFFFF)
    assert d["nodes"][0, 0] == 48 and k > 16, k
    parents, pruned, worst = _check_pruned_sums(d, 0.15)
    print("wide root: %d root children, %d parents, %d pruned, largest relative difference %.3e" %
          (k, parents, pruned, worst))
    assert pruned >= 1


# cpuct found by trying a few values per board: the root passes 64 children and the visits the
# desired-per-child rule forces down low-prior children are pruned somewhere in the tree (at 7x7
# at the root itself: 67 children, 2e-3 of its weight)
WIDE_VISITS, WIDE_CAP = 380, 384


@pytest.mark.parametrize("X,Y,W,cpuct", [(7, 7, 5, 96.0), (9, 9, 5, 48.0)], ids=["7x7", "9x9"])
def test_recompute_obeys_the_pruning_past_64_children(X, Y, W, cpuct):
    """A root past 64 children (desired per-child visits plus noise spread the visits): the scan
    order crosses the lanes' items, on the four- and seven-item computeLevel."""
    an, _ = _analysis(X, Y, W, visits=WIDE_VISITS, cap=WIDE_CAP, expl=PRUNE, cpuct_exploration=cpuct,
                      root_desired_per_child_visits_coeff=4.0, **SUMS, **NOISE)
    _run(an, [dict(id=1, moves=[])])
    d = _dump(an, WIDE_CAP)
    an.close()
    k = int(d["nodes"][0, 10] & 0xFFFF)
    assert d["nodes"][0, 0] == WIDE_VISITS and k > 64, k
    parents, pruned, worst = _check_pruned_sums(d, 0.15)
    print("%dx%d: %d root children, %d parents, %d pruned, largest relative difference %.3e" %
          (X, Y, k, parents, pruned, worst))
    assert pruned >= 1 and d["nodes"][0, 1] != _bits(_f(0))  # the root itself was scanned


# ---------------------------------------------------------------------------------------
# 6. The descent obeys the factor.

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


def _select_best(d, i, sp, expl, P):
    """selectBest (search.hip; selectBestChildToDescend searchexplorehelpers.cpp:304-451) on node i
    of a dump in np.float32, in the kernel's operation order.  Returns (slot, new move or -1);
    slot == numChildren: a new child."""
    nodes, edges = d["nodes"], d["edges"]
    is_root = i == 0
    k = int(nodes[i, 10] & 0xFFFF)
    pla = int(nodes[i, 10] >> 16) & 0xFF
    rec = _f32(nodes[i, 1:8])  # ws, wsq, u, usq, wl, nnWin, nnLoss
    moves = edges[i, :k, 2].astype(np.int64)
    pol = d["root_policy"]
    p = (pol[moves] if is_root else d["priors"][i, :k]).astype(np.float32)
    ci = edges[i, :k, 0].astype(np.int64)
    cvis = nodes[ci, 0]
    cws, cu = _f32(nodes[ci, 1]), _f32(nodes[ci, 3])
    probs = [_f(0) if p[j] < 0 else p[j] for j in range(k)]
    cw = [_f(0) if p[j] < 0 else _child_weight(edges[i, j, 1], cvis[j], cws[j]) for j in range(k)]
    prob_mass, total = _tree_sum64(probs), _tree_sum64(cw)
    # fpuValue
    parent_u = rec[2]
    for_fpu = parent_u
    if sp.fpu_parent_weight_by_visited_policy:
        assert sp.fpu_parent_weight_by_visited_policy_pow == 2.0
        avg_w = min(_f(1), _f(prob_mass * prob_mass))
        for_fpu = _f(_f(avg_w * parent_u) + _f(_f(_f(1) - avg_w) * _f(rec[5] - rec[6])))
    red_max = _f(sp.root_fpu_reduction_max if is_root else sp.fpu_reduction_max)
    loss_prop = _f(sp.root_fpu_loss_prop if is_root else sp.fpu_loss_prop)
    reduction = _f(red_max * np.sqrt(prob_mass))
    fpu = _f(for_fpu - reduction) if pla == 2 else _f(for_fpu + reduction)
    loss_value = _f(-1) if pla == 2 else _f(1)
    fpu = _f(fpu + _f(_f(loss_value - fpu) * loss_prop))
    # exploreScaling and the factor
    assert sp.cpuct_exploration_log == 0.0
    scaling = _f(_f(sp.cpuct_exploration) * np.sqrt(_f(total + _f(0.01))))
    scaling = _f(scaling * _stdev_factor(int(nodes[i, 0]), rec[0], rec[2], rec[3], expl["cpuct_utility_stdev_prior"],
                                         expl["cpuct_utility_stdev_prior_weight"], expl["cpuct_utility_stdev_scale"]))
    best, best_slot = -np.inf, -1
    coeff = _f(sp.root_desired_per_child_visits_coeff)
    for j in range(k):
        if p[j] < 0:
            continue
        w = cw[j]
        u = fpu if (cvis[j] == 0 or w <= 0) else cu[j]
        if is_root and coeff > 0 and p[j] > 0 and w < np.sqrt(_f(_f(p[j] * total) * coeff)):
            val = _f(1e20)
        else:
            val = _f(_f(_f(scaling * p[j]) / _f(_f(1) + w)) + (u if pla == 2 else -u))
        if val > best:
            best, best_slot = val, j
    bp, bpos = _f(-1), -1
    if is_root:
        has = np.zeros(P, bool)
        has[moves] = True
        for pos in range(P):
            if not has[pos] and pol[pos] >= 0 and pol[pos] > bp:
                bp, bpos = pol[pos], pos
    elif int(d["next_pos"][i]) != 0xFFFF:
        bp, bpos = d["next_prior"][i], int(d["next_pos"][i])
    new_pos = -1
    if bpos >= 0:
        val = _f(_f(_f(scaling * bp) / _f(1)) + (fpu if pla == 2 else -fpu))
        if val > best:
            best_slot, new_pos = k, bpos
    return best_slot, new_pos


def test_descent_obeys_the_factor(game_moves):
    P = 100
    an, sp = _analysis(expl=FACTOR, cpuct_exploration_log=0.0, fpu_parent_weight_by_visited_policy_pow=2.0)
    an.submit([dict(id=1, moves=game_moves[:8])])
    prev = None
    levels = differ = playouts = 0
    plain = dict(FACTOR, cpuct_utility_stdev_scale=0.0)
    for _ in range(VISITS + 8):
        an.step(1)
        cur = _dump(an)
        if len(cur["nodes"]) == 0 or cur["nodes"][0, 0] == 0:
            continue
        if cur["nodes"][0, 0] >= VISITS - 2:
            break  # before the visit limit: the slot still holds this tree
        if prev is not None and cur["nodes"][0, 0] == prev["nodes"][0, 0] + 1:
            playouts += 1
            pp, cp = _paths(prev["nodes"], prev["edges"]), _paths(cur["nodes"], cur["edges"])
            cidx = {path: j for j, path in enumerate(cp)}
            # the playout's path: the nodes of the previous tree whose visits rose, root first
            path = [j for j in range(len(pp)) if cur["nodes"][cidx[pp[j]], 0] > prev["nodes"][j, 0]]
            path.sort(key=lambda j: len(pp[j]))
            assert path and path[0] == 0 and [len(pp[j]) for j in path] == list(range(len(path)))
            for depth, j in enumerate(path):
                if int(prev["nodes"][j, 10] >> 24) & 2:
                    assert depth == len(path) - 1  # a terminal node ends the descent
                    continue
                c = cidx[pp[j]]
                k = int(prev["nodes"][j, 10] & 0xFFFF)
                rose = [s for s in range(k) if cur["edges"][c, s, 1] > prev["edges"][j, s, 1]]
                k_now = int(cur["nodes"][c, 10] & 0xFFFF)
                taken = rose[0] if rose else k
                assert len(rose) == (0 if k_now == k + 1 else 1) and k_now in (k, k + 1), (depth, rose, k, k_now)
                slot, new_pos = _select_best(prev, j, sp, FACTOR, P)
                assert slot == taken, (playouts, depth, slot, taken)
                if taken == k:
                    assert new_pos == cur["edges"][c, k, 2]
                    assert depth == len(path) - 1  # an expansion ends the descent
                levels += 1
                differ += _select_best(prev, j, sp, plain, P) != (slot, new_pos)
        prev = cur
    an.close()
    print("%d playouts, %d levels restated, %d where factor 1 chooses another child" % (playouts, levels, differ))
    assert playouts >= 40 and levels >= 80
    assert differ >= 1  # otherwise the case does not tell the two rules apart


# ---------------------------------------------------------------------------------------
# 7. Play selection.

def test_play_selection_follows_the_scaled_exploration(game_moves):
    an, sp = _analysis(expl=FACTOR, cpuct_exploration_log=0.0, use_lcb_for_selection=0, **NOISE)
    h, m = _run(an, [dict(id=1, moves=game_moves[:8])])
    d = _dump(an)
    an.close()
    nodes, edges, pol = d["nodes"], d["edges"], d["root_policy"]
    k = int(nodes[0, 10] & 0xFFFF)
    pla = int(nodes[0, 10] >> 16) & 0xFF
    m = m[0][:k]
    rec = _f32(nodes[0, 1:8])
    ci = edges[0, :k, 0].astype(np.int64)
    cvis, cws, cu = nodes[ci, 0], _f32(nodes[ci, 1]), _f32(nodes[ci, 3])
    moves = edges[0, :k, 2].astype(np.int64)
    cw = [_child_weight(edges[0, j, 1], cvis[j], cws[j]) for j in range(k)]
    total = _tree_sum64(cw)

    def values(scale):
        best_i, max_good = 0, _f(-1e30)
        for j in range(k):
            ev = _f(edges[0, j, 1])
            gdn = _f(_f(_f(cw[j] * max(_f(0), _f(ev - _f(1)))) / max(_f(1), ev)) + _f(_f(2) * pol[moves[j]]))
            if gdn > max_good:
                max_good, best_i = gdn, j
        # fpuValue(root, probMass 1)
        for_fpu = rec[2]
        if sp.fpu_parent_weight_by_visited_policy:
            for_fpu = _f(_f(_f(1) * rec[2]) + _f(_f(0) * _f(rec[5] - rec[6])))
        red = _f(_f(sp.root_fpu_reduction_max) * np.sqrt(_f(1)))
        fpu = _f(for_fpu - red) if pla == 2 else _f(for_fpu + red)
        fpu = _f(fpu + _f(_f((_f(-1) if pla == 2 else _f(1)) - fpu) * _f(sp.root_fpu_loss_prop)))
        scaling = _f(_f(sp.cpuct_exploration) * np.sqrt(_f(total + _f(0.01))))
        scaling = _f(scaling * _stdev_factor(int(nodes[0, 0]), rec[0], rec[2], rec[3], 0.40, 2.0, scale))
        bp, bw = pol[moves[best_i]], cw[best_i]
        bu = fpu if (cvis[best_i] == 0 or bw <= 0) else cu[best_i]
        best_value = -np.inf if bp < 0 else _f(_f(_f(scaling * bp) / _f(_f(1) + bw)) + (bu if pla == 2 else -bu))
        vals = list(cw)
        for j in range(k):
            if j == best_i:
                continue
            w = cw[j]
            if cvis[j] == 0 or w <= 0:
                reduced = _f(0)
            else:
                p = pol[moves[j]]
                if p < 0:
                    wanted = _f(0)
                else:
                    explore = _f(best_value - (cu[j] if pla == 2 else -cu[j]))
                    wanted = _f(np.inf) if explore <= 0 else max(_f(0), _f(_f(_f(scaling * p) / explore) - _f(1)))
                reduced = wanted if w > wanted else w
            vals[j] = np.ceil(reduced)
        vals = np.array(vals, np.float32)
        mx = vals.max()
        sub, prune = min(_f(sp.chosen_move_subtract), _f(mx / _f(64))), min(_f(sp.chosen_move_prune), _f(mx / _f(64)))
        out = np.where(vals < prune, _f(0), np.maximum(_f(0), (vals - sub).astype(np.float32)))
        return out.astype(np.float32)

    want, plain = values(0.85), values(0.0)
    np.testing.assert_array_equal(_bits(m["play_selection_value"]), _bits(want))
    assert not np.array_equal(want, plain)  # the factor shows in the reduced weights


# ---------------------------------------------------------------------------------------
# 8. Fused against separate rounds.

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
    sp.set_exploration(**BOTH)
    return sp


@pytest.mark.parametrize("ci", [3, 16])
def test_fused_rounds_match_separate_rounds(ci):
    G = 32
    kw = dict(num_games=G, max_visits=48, seed=61, node_cap=CAP, commit_interval=ci, nn_cache_log2=10)
    a, b = _selfplay(True, **kw), _selfplay(False, **kw)
    a.enable_timing(1)
    b.enable_timing(1)
    done = 0
    for chunk in [5, 40, 700]:
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
# 9. Match, per side.

def test_match_sides_carry_their_own_setting():
    X, Y, W, G = 5, 5, 4, 4
    base = dict(max_visits=32, use_graph_search=0, root_num_symmetries_to_sample=1, root_noise_enabled=1,
                chosen_move_subtract=0.0, chosen_move_prune=0.0, **SUMS)
    mt = kc.Match(X, Y, W, num_games=G, seed=SEED, node_cap=128, share_net=True,
                  search=kc.default_match_params(**base), sides=(dict(base), dict(base)))
    with pytest.raises(kc.CoffeeError, match="side"):
        mt.set_exploration(side=-1, **PRUNE)
    with pytest.raises(kc.CoffeeError, match="side"):
        mt.set_exploration(side=2, **PRUNE)
    mt.set_exploration(side=0, **PRUNE)
    mt.set_exploration(side=1)
    seen = {0: 0, 1: 0}
    pruned = {0: 0, 1: 0}
    for _ in range(120):
        mt.step(1)
        for g in range(G):
            i = mt.game_info(g)
            if i["phase"] != 1:
                continue
            nodes, edges = mt.game_tree(g, 128)
            if len(nodes) == 0 or nodes[0, 0] < 24:
                continue
            priors, next_prior, next_pos = mt.game_tree_priors(g, 128)
            # the side that searches: the candidate (side 1) is black in game n of slot s iff s + n is even
            side = 1 if i["pla"] == (1 if (g + i["gameNum"]) % 2 == 0 else 2) else 0
            d = dict(nodes=nodes, edges=edges, priors=priors, root_policy=mt.root_policy(g))
            _, p, _ = _check_pruned_sums(d, 0.15, prune=side == 0)
            seen[side] += 1
            pruned[side] += p
        if min(seen.values()) >= 8 and pruned[0] >= 1:
            break
    mt.close()
    print("trees checked per side: %s, pruned parents per side: %s" % (seen, pruned))
    assert min(seen.values()) >= 8 and pruned[0] >= 1 and pruned[1] == 0
    # an engine without per-side settings takes -1 only
    mt = kc.Match(X, Y, W, num_games=G, seed=SEED, node_cap=128, search=kc.default_match_params(max_visits=8))
    for side in (0, 1):
        with pytest.raises(kc.CoffeeError, match="side"):
            mt.set_exploration(side=side, **PRUNE)
    mt.set_exploration(**BOTH)
    mt.step(40)
    assert mt.stats()["errors"] == 0
    mt.close()


# ---------------------------------------------------------------------------------------
# 10. Commands.

def _winrate(white_wl, pla):
    w = 0.5 * (max(-1.0, min(1.0, float(white_wl))) + 1.0)
    return w if pla == 2 else 1.0 - w


def test_analysis_command_reads_the_config_keys():
    cmd = [os.path.join(REPO, "katacoffee_amd", "katago"), "analysis", "-config",
           os.path.join(REPO, "configs", "analysis_coffee5.cfg"), "-override-config",
           "maxVisits=48,numAnalysisSlots=2,nnCacheSizePowerOfTwo=0,cpuctUtilityStdevScale=0.85,useNoisePruning=true,"
           "noisePruneUtilityScale=0.15,noisePruningCap=1e50"]
    r = subprocess.run(cmd, input='{"id":"a","moves":[]}\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip())
    got = {}
    for on in (0, 1):
        an = kc.Analysis(5, 5, 4, num_slots=2, seed=1, search=kc.default_analysis_params(max_visits=48))
        if on:
            an.set_exploration(**BOTH)
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
    bad = subprocess.run(cmd[:-1] + ["cpuctUtilityStdevScale=7"], input="", capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "cpuctUtilityStdevScale" in bad.stderr


def test_match_command_accepts_per_bot_keys(tmp_path):
    katago = os.path.join(REPO, "katacoffee_amd", "katago")
    model = str(tmp_path / "b2c32.cfnn")
    kc.write_random_model("b2c32", 0xBEEF, model)
    r = subprocess.run([katago, "match", "-config", os.path.join(REPO, "configs", "match_coffee5.cfg"),
                        "-sgf-output-dir", str(tmp_path / "sgf"), "-override-config",
                        "nnModelFile=%s,numGamesTotal=4,numGameThreads=4,maxVisits0=8,maxVisits1=8,seed=7,"
                        "nnCacheSizePowerOfTwo=10,nnPrecision=accurate,cpuctUtilityStdevScale0=0.85,"
                        "useNoisePruning1=true,noisePruneUtilityScale1=0.3" % model],
                       capture_output=True, text=True, timeout=120)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log
    assert "bot 0: cpuct stdev scale 0.85" in log and "noise pruning off" in log, log
    assert "bot 1: cpuct stdev scale 0" in log and "noise pruning on" in log, log
    bad = subprocess.run([katago, "match", "-config", os.path.join(REPO, "configs", "match_coffee5.cfg"),
                          "-sgf-output-dir", str(tmp_path / "sgf2"), "-override-config", "noisePruneUtilityScale1=0"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "noisePruneUtilityScale1" in (bad.stdout + bad.stderr)
