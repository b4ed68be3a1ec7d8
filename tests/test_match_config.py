"""Two-network match play, the checks that need no GPU: the config is validated before
the first device call, the defaults are gatekeeper1.cfg's, and the scoring is right."""
import ctypes

import numpy as np
import pytest

import katacoffee_amd as kc


@pytest.fixture(scope="module")
def L():
    import os
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


def _create(L, X=5, Y=5, W=4, **search_over):
    cfg = kc.MatchConfig()
    cfg.x, cfg.y, cfg.win_len = X, Y, W
    cfg.num_games = 4
    cfg.node_cap = 64
    cfg.seed = 1
    cfg.search = kc.default_match_params(max_visits=8, **search_over)
    h = ctypes.c_void_p()
    rc = L.coffee_match_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, L.coffee_last_error().decode(), h


# every setting that keeps a tree across moves or exists only to make training rows
FORBIDDEN = [("cheap_search_prob", 0.25), ("reduce_visits", 1), ("early_fork_game_prob", 0.04),
             ("fork_game_prob", 0.01), ("side_position_prob", 0.02), ("record_tree_positions", 1),
             ("policy_surprise_data_weight", 0.5), ("value_surprise_data_weight", 0.1)]


@pytest.mark.parametrize("name,value", FORBIDDEN, ids=[n for n, _ in FORBIDDEN])
def test_forbidden_setting_is_rejected_by_name(L, name, value):
    rc, msg, h = _create(L, **{name: value})
    assert rc == -1, (rc, msg)  # COFFEE_EINVAL
    assert name in msg, msg
    assert not h.value


@pytest.mark.parametrize("geom,word", [((11, 5, 4), "board size"), ((5, 1, 4), "board size"), ((5, 5, 9), "win_len"),
                                       ((5, 5, 1), "win_len")])
def test_bad_geometry_is_rejected(L, geom, word):
    rc, msg, h = _create(L, *geom)
    assert rc == -1 and word in msg, (rc, msg)
    assert not h.value


def test_python_class_raises_the_same_error(L):
    with pytest.raises(kc.CoffeeError, match="cheap_search_prob"):
        kc.Match(5, 5, 4, num_games=2, cheap_search_prob=0.5)


def test_match_params_default_values(L):
    p = kc.default_match_params()
    # gatekeeper1.cfg:49, :72-80, :95-106
    assert p.max_visits == 150
    assert p.root_noise_enabled == 0
    assert p.chosen_move_temperature_early == pytest.approx(0.5)
    assert p.chosen_move_temperature == pytest.approx(0.2)
    assert p.chosen_move_temperature_halflife == pytest.approx(19.0)
    assert p.chosen_move_subtract == 0.0 and p.chosen_move_prune == pytest.approx(1.0)
    assert p.use_lcb_for_selection == 1
    assert p.lcb_stdevs == pytest.approx(5.0) and p.min_visit_prop_for_lcb == pytest.approx(0.15)
    assert p.cpuct_exploration == pytest.approx(1.1) and p.cpuct_exploration_log == 0.0
    assert p.fpu_reduction_max == pytest.approx(0.2) and p.root_fpu_reduction_max == pytest.approx(0.1)
    assert p.value_weight_exponent == pytest.approx(0.5)
    assert p.subtree_value_bias_factor == pytest.approx(0.35)
    assert p.subtree_value_bias_weight_exponent == pytest.approx(0.8)
    assert p.use_graph_search == 1
    # all play settings off
    assert p.cheap_search_prob == 0.0 and p.reduce_visits == 0
    assert p.policy_surprise_data_weight == 0.0 and p.value_surprise_data_weight == 0.0
    assert p.init_games_with_policy == 0
    assert p.early_fork_game_prob == 0.0 and p.fork_game_prob == 0.0
    assert p.side_position_prob == 0.0 and p.record_tree_positions == 0
    # and the defaults themselves pass the validation they are meant for: the next failure
    # of a create without a device is a HIP one (-2), or none where a GPU is present
    rc, msg, h = _create(L)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        L.coffee_match_destroy(h)


def test_match_score(L):
    # (slot, game number, moves, winner, candidate's colour)
    header = np.array([[0, 0, 9, 1, 1],    # candidate black, black wins: candidate 1
                       [1, 0, 12, 2, 2],   # candidate white, white wins: candidate 1
                       [2, 0, 25, 0, 1],   # draw: half each
                       [3, 0, 7, 2, 1],    # candidate black, white wins: baseline 1
                       [4, 0, 8, 1, 2]],   # candidate white, black wins: baseline 1
                      np.int32)
    assert kc.match_score(header[:1]) == (1.0, 0.0)
    assert kc.match_score(header[1:2]) == (1.0, 0.0)
    assert kc.match_score(header[2:3]) == (0.5, 0.5)
    assert kc.match_score(header) == (2.5, 2.5)
    assert kc.Match.score(header[3:]) == (0.0, 2.0)
    assert kc.match_score(header[:0]) == (0.0, 0.0)
    bad = header[:1].copy()
    bad[0, 4] = 0  # no candidate colour: not a match record
    with pytest.raises(kc.CoffeeError):
        kc.match_score(bad)
