"""GPU parity of the search kernels' fast paths against the CPU oracle, bit-exact (game
state, canonical search trees, root priors, training rows), the way test_gpu_parity.py
compares them:

  level forms   a path level whose node has at most 64 children takes the one-item form
                of the selection, a wider one the two-item form: a run in which a root
                passes 64 children while every other node stays below uses both
  rare leaves   policy-init moves, fork candidates, side positions and root evaluations
                run out of line of the round kernels; the edge pool grows at a node's
                17th child
  bitboards     geometries of at most 64 cells use one-word bitboards; 9x9 keeps two words
"""
import os

import numpy as np
import pytest

import katacoffee_amd as kc
from oracle import oracle

pytestmark = pytest.mark.gpu

INFO_KEYS = [("phase", "phase"), ("rootK", "rootK"), ("liveCount", "nodeCount"), ("gameNum", "gameNum"),
             ("turn", "turn"), ("pla", "pla"), ("playouts", "playouts"), ("nnEvals", "nnEvals"),
             ("moves", "movesMade"), ("gamesFinished", "gamesFinished"), ("rngCtr", "rngCtr"),
             ("lastCell", "lastCell"), ("lastDir", "lastDir")]

# selfplay1.cfg's play settings with the visit counts scaled to 32 visits, policy-init
# openings, side positions, and forks at rates high enough for a short run
PRODUCTION = dict(cheap_search_prob=0.75, cheap_search_visits=10, cheap_search_target_weight=0.0, reduce_visits=1,
                  reduce_visits_threshold=0.9, reduce_visits_threshold_lookback=3, reduced_visits_min=10,
                  reduced_visits_weight=0.1, policy_surprise_data_weight=0.5, value_surprise_data_weight=0.1,
                  init_games_with_policy=1, side_position_prob=0.2,
                  early_fork_game_prob=0.5, early_fork_game_expected_move_prop=0.2, fork_game_prob=0.5,
                  fork_game_min_choices=2, early_fork_game_max_choices=5, fork_game_max_choices=7)


def _engine(fused, X, Y, W, **kw):
    # the engine reads COFFEE_FUSED_ROUNDS when it is created
    old = os.environ.pop("COFFEE_FUSED_ROUNDS", None)
    os.environ["COFFEE_FUSED_ROUNDS"] = "1" if fused else "0"
    try:
        return kc.Selfplay(X, Y, W, **kw)
    finally:
        os.environ.pop("COFFEE_FUSED_ROUNDS", None)
        if old is not None:
            os.environ["COFFEE_FUSED_ROUNDS"] = old


def _sorted_rows(r):
    order = np.lexsort((r["meta"][:, 2], r["meta"][:, 1], r["meta"][:, 0]))
    return {k: v[order] for k, v in r.items()}


def _children(nodes):
    return (nodes[:, 10] & 0xFFFF).astype(np.int64)  # Node::numChildren; row 0 is the root


def _run(gpu, ora, games, chunks):
    """Steps both engines through `chunks` (cumulative rounds), comparing every game at each
    stop; returns the oracle's trees' widest root and widest other node over the stops."""
    done = 0
    root_k = other_k = 0
    for chunk in chunks:
        gpu.step(chunk - done)
        ora.rounds(chunk - done)
        done = chunk
        for g in range(games):
            gi, oi = gpu.game_info(g), ora.info(g)
            for a, b in INFO_KEYS:
                assert gi[a] == oi[b], (done, g, a, gi[a], oi[b])
            gn, ge = gpu.game_tree(g)
            on, oe = ora.game_tree(g)
            np.testing.assert_array_equal(gn, on, err_msg="round %d game %d nodes" % (done, g))
            np.testing.assert_array_equal(ge, oe, err_msg="round %d game %d edges" % (done, g))
            if gi["phase"] == 1:
                np.testing.assert_array_equal(gpu.root_policy(g), ora.root_noised(g))
            if len(on):
                k = _children(on)
                root_k = max(root_k, int(k[0]))
                other_k = max(other_k, int(k[1:].max()) if len(k) > 1 else 0)
    return root_k, other_k


def _compare_rows(gpu, ora):
    st = gpu.stats()
    assert st["errors"] == 0 and st["rows_dropped"] == 0 and st["games_finished"] > 0
    gr, orr = _sorted_rows(gpu.drain_rows()), _sorted_rows(ora.rows())
    assert len(gr["meta"]) == len(orr["meta"]) > 0
    for k in orr:
        np.testing.assert_array_equal(gr[k], orr[k], err_msg=k)
    return orr


# 256 visits with cpuct 16 spread an empty 5x5 board's first search (100 legal moves) over
# more than 64 root children -- found with the oracle alone: 71 at 240 visits -- while no
# other node passes 10.  Stops at rounds 200 and 290 fall into those first searches (the
# staggered starts end by round 37), before and after the root's 65th child.
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_both_level_forms_bit_exact_vs_oracle(fused):
    games, visits, cap, seed, rounds = 8, 256, 320, 5, 6000
    play = dict(cpuct_exploration=16.0)
    gpu = _engine(fused, 5, 5, 4, num_games=games, max_visits=visits, seed=seed, node_cap=cap, commit_interval=16,
                  start_stagger=37, nn_cache_log2=0, row_capacity=1 << 15, **play)
    gpu.enable_timing(1)
    ora = oracle.Selfplay(5, 5, 4, games=games, max_visits=visits, node_cap=cap, seed=seed, nn_cache_log2=0,
                          commit_interval=16, start_stagger=37, **play)
    root_k, other_k = _run(gpu, ora, games, [1, 40, 200, 290, 700, rounds])
    # both forms ran: the oracle's trees held a root past 64 children (two-item form) and
    # every other node at or below 64 (one-item form)
    assert root_k > 64 and 0 < other_k <= 64, (root_k, other_k)
    _compare_rows(gpu, ora)
    fused_launches = gpu.kernel_time(4)[1]
    assert (fused_launches > rounds // 2) if fused else (fused_launches == 0), fused_launches
    gpu.close()


# 16 games x 32 visits at production play settings.  Seed and node cap found with the oracle
# alone: in this run finished games hold policy-init moves, forked games and side-position
# rows, and a kept subtree's root reaches 18 children (the edge-pool block is allocated at
# the 17th).  Both the separate backup kernel and the fused one call the rare leaf kinds.
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_rare_leaves_out_of_line_bit_exact_vs_oracle(fused):
    games, visits, cap, seed = 16, 32, 64, 2
    gpu = _engine(fused, 5, 5, 4, num_games=games, max_visits=visits, seed=seed, node_cap=cap, commit_interval=16,
                  start_stagger=37, nn_cache_log2=10, row_capacity=1 << 15, **PRODUCTION)
    ora = oracle.Selfplay(5, 5, 4, games=games, max_visits=visits, node_cap=cap, seed=seed, nn_cache_log2=10,
                          commit_interval=16, start_stagger=37, **PRODUCTION)
    root_k, other_k = _run(gpu, ora, games, [1, 20, 60, 100, 150, 200, 300, 400, 600, 900, 1200])
    rows = _compare_rows(gpu, ora)
    gt = rows["globalTargetsNC"]
    # from the oracle's run: [55] game mode (2 = forked game), [53] the game's start turn
    # (> 0 in an unforked game: policy-init moves), [27] = 0 only in side-position rows
    assert (gt[:, 55] == 2).sum() > 0, "no forked game"
    assert ((gt[:, 55] == 0) & (gt[:, 53] > 0)).sum() > 0, "no policy-init move"
    assert (gt[:, 27] == 0).sum() > 0, "no side position"
    assert max(root_k, other_k) >= 17, "no edge-pool growth"
    gpu.close()


# 9x9 (81 cells, P = 324): the two-word bitboards, still exercised now that 5x5 and 7x7
# take the one-word form.
def test_two_word_bitboards_bit_exact_vs_oracle():
    games, visits, cap, seed, rounds = 4, 64, 128, 7, 5000
    gpu = kc.Selfplay(9, 9, 5, num_games=games, max_visits=visits, seed=seed, node_cap=cap, commit_interval=1,
                      nn_cache_log2=0, row_capacity=1 << 15)
    ora = oracle.Selfplay(9, 9, 5, games=games, max_visits=visits, node_cap=cap, seed=seed, nn_cache_log2=0)
    _run(gpu, ora, games, [1, 7, 200, rounds])
    _compare_rows(gpu, ora)
    gpu.close()
