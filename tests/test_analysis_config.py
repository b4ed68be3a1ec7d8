"""Position analysis, the checks that need no GPU: a config is validated before the first
device call with the offending field named, the defaults are analysis_example.cfg's, and a
query's host-side checks name the field."""
import ctypes
import os

import pytest

import katacoffee_amd as kc


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


def _create(L, X=5, Y=5, W=4, num_slots=4, query_capacity=8, max_pv_len=8, **search_over):
    cfg = kc.AnalysisConfig()
    cfg.x, cfg.y, cfg.win_len = X, Y, W
    cfg.num_slots = num_slots
    cfg.node_cap = 64
    cfg.seed = 1
    cfg.query_capacity = query_capacity
    cfg.max_pv_len = max_pv_len
    cfg.search = kc.default_analysis_params(max_visits=8, **search_over)
    h = ctypes.c_void_p()
    rc = L.coffee_analysis_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, L.coffee_last_error().decode(), h


# match play's list, plus the opening moves a query makes pointless
FORBIDDEN = [("cheap_search_prob", 0.25), ("reduce_visits", 1), ("early_fork_game_prob", 0.04),
             ("fork_game_prob", 0.01), ("side_position_prob", 0.02), ("record_tree_positions", 1),
             ("policy_surprise_data_weight", 0.5), ("value_surprise_data_weight", 0.1),
             ("init_games_with_policy", 1)]


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


@pytest.mark.parametrize("field,value", [("max_pv_len", 17), ("max_pv_len", -1), ("query_capacity", 0),
                                         ("query_capacity", -3), ("num_slots", 0)])
def test_bad_engine_field_is_rejected_by_name(L, field, value):
    rc, msg, h = _create(L, **{field: value})
    assert rc == -1 and field in msg, (rc, msg)
    assert not h.value


def test_python_class_raises_the_same_error(L):
    with pytest.raises(kc.CoffeeError, match="init_games_with_policy"):
        kc.Analysis(5, 5, 4, num_slots=2, init_games_with_policy=1)
    with pytest.raises(kc.CoffeeError, match="max_pv_len"):
        kc.Analysis(5, 5, 4, num_slots=2, max_pv_len=kc.ANALYSIS_MAX_PV + 1)


def test_analysis_params_default_values(L):
    p, m = kc.default_analysis_params(), kc.default_match_params()
    # analysis_example.cfg:66, :278-285
    assert p.max_visits == 500
    assert p.use_lcb_for_selection == 1
    assert p.lcb_stdevs == pytest.approx(5.0) and p.min_visit_prop_for_lcb == pytest.approx(0.15)
    assert p.root_num_symmetries_to_sample == 1 and p.root_noise_enabled == 0
    assert p.chosen_move_subtract == 0.0 and p.chosen_move_prune == 0.0  # unpruned play-selection values
    # everything else is the match default
    for name, _ in kc.SearchParams._fields_:
        if name not in ("max_visits", "chosen_move_prune"):
            assert getattr(p, name) == getattr(m, name), name
    # the defaults pass their own validation: the next failure without a device is a HIP one
    rc, msg, h = _create(L)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        L.coffee_analysis_destroy(h)


def test_query_checks_name_the_field(L):
    kc.analysis_query_check(5, 5, 4, dict(id=1, moves=list(range(25))))  # a full board of moves is fine
    with pytest.raises(kc.CoffeeError, match="num_moves"):
        kc.analysis_query_check(5, 5, 4, dict(id=1, moves=[0] * 26))  # num_moves > A
    with pytest.raises(kc.CoffeeError, match=r"moves\[2\]"):
        kc.analysis_query_check(5, 5, 4, dict(id=1, moves=[0, 99, 100]))  # a move >= P
    kc.analysis_query_check(6, 4, 3, dict(id=1, moves=[95]))
    with pytest.raises(kc.CoffeeError, match=r"moves\[0\]"):
        kc.analysis_query_check(6, 4, 3, dict(id=1, moves=[96]))
    with pytest.raises(kc.CoffeeError, match="max_visits"):
        kc.analysis_query_check(5, 5, 4, dict(id=1, moves=[], max_visits=-1))
    q = kc.analysis_queries([dict(id=7, moves=[3])])
    q["num_moves"] = -1
    with pytest.raises(kc.CoffeeError, match="num_moves"):
        kc.analysis_query_check(5, 5, 4, q)
    with pytest.raises(kc.CoffeeError, match="board size"):
        kc.analysis_query_check(11, 5, 4, dict(id=1, moves=[]))


def test_query_defaults(L):
    q = kc.analysis_queries([dict(id=(5 << 32) | 9, moves=[1, 2]), dict(id=3, moves=[], stream=8, game_num=2,
                                                                       rng_counter=31, max_visits=50)])
    assert q[0]["stream"] == 9 and q[0]["game_num"] == 0 and q[0]["rng_counter"] == 0 and q[0]["max_visits"] == 0
    assert q[0]["num_moves"] == 2 and list(q[0]["moves"][:3]) == [1, 2, 0]
    assert (q[1]["stream"], q[1]["game_num"], q[1]["rng_counter"], q[1]["max_visits"]) == (8, 2, 31, 50)
