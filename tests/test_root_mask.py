"""The root restriction rule on the host (kc.root_mask / kc.symmetry_move, the code the
analysis kernels run) against its numpy restatement in
tests/helpers/root_mask_cases.py.  No device."""
import importlib.util
import os

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("root_mask_cases",
                                               os.path.join(REPO, "tests", "helpers", "root_mask_cases.py"))
rc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rc)

CASES = rc.cases()


@pytest.fixture(scope="module", autouse=True)
def L():
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


def run(X, Y, W, moves, **kw):
    avoid, allow = kw.get("avoid"), kw.get("allow")
    e = rc.expected(X, Y, W, moves, avoid=avoid, allow=allow, prune=kw.get("prune", True))
    col, hc, hd = rc.library_inputs(e["board"], e["hist"])
    r = kc.root_mask(X, Y, W, col, hc, hd, e["legal"], avoid_moves=avoid, allow_moves=allow,
                     prune=kw.get("prune", True))
    return e, r


def check(e, r):
    assert r["symmetries"] == e["used"]
    np.testing.assert_array_equal(r["mask"], e["mask"])
    keep = e["legal"] & ~r["mask"]
    assert r["left"] == int(keep.sum()) and r["num_masked"] == int((e["legal"] & e["mask"]).sum())
    # exactly one survivor per orbit: its lowest position
    assert sorted(np.nonzero(keep)[0].tolist()) == sorted(e["orbits"])
    for low, orb in e["orbits"].items():
        assert [p for p in orb if keep[p]] == [low]


def test_symmetry_move_matches_the_restatement():
    for X, Y in [(5, 5), (7, 7), (9, 9), (6, 4), (10, 10)]:
        for s in range(8 if X == Y else 4):
            for p in range(4 * X * Y):
                assert kc.symmetry_move(X, Y, s, p) == rc.image(X, Y, s, p), (X, Y, s, p)
    with pytest.raises(kc.CoffeeError):
        kc.symmetry_move(5, 5, 8, 0)
    with pytest.raises(kc.CoffeeError):
        kc.symmetry_move(5, 5, 0, 100)


@pytest.mark.parametrize("name,X,Y,W", [("empty5", 5, 5, 4), ("empty7", 7, 7, 5), ("empty9", 9, 9, 5),
                                        ("empty6x4", 6, 4, 3)])
def test_empty_boards(name, X, Y, W):
    e, r = run(X, Y, W, [])
    assert r["symmetries"] == (list(range(8)) if X == Y else list(range(4)))
    check(e, r)
    assert r["left"] == len(e["orbits"])
    if name == "empty5":
        # the 100 positions fall into 18 orbits (Burnside: (100 + 4 + 4 * 10) / 8);
        # one of them, the four corner diagonals that leave the board at once, is illegal
        assert int(e["legal"].sum()) == 96 and r["left"] == 17
    # without pruning nothing is masked, and the symmetries are reported all the same
    e0, r0 = run(X, Y, W, [], prune=False)
    assert not r0["mask"].any() and r0["symmetries"] == e["used"] and r0["left"] == int(e["legal"].sum())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cases_match_the_restatement(case):
    _, X, Y, W, moves = case
    check(*run(X, Y, W, moves))


def test_symmetric_one_move_positions():
    # a centre move keeps the symmetries that keep its direction; a corner move along its
    # diagonal keeps the transpose
    want = {0: [0, 1, 2, 3], 1: [0, 1, 2, 3], 2: [0, 3, 4, 7], 3: [0, 3, 4, 7]}
    for d in range(4):
        e, r = run(5, 5, 4, [d * 25 + 12])
        assert r["symmetries"] == e["used"] == want[d], d
    e, r = run(5, 5, 4, [2 * 25 + 0])
    assert r["symmetries"] == e["used"] == [0, 4]


def test_cases_hold_trivial_and_nontrivial_groups():
    sizes = [len(rc.expected(X, Y, W, moves)["used"]) for _, X, Y, W, moves in CASES]
    assert sum(n > 1 for n in sizes) >= 3 and sum(n == 1 for n in sizes) >= 3, sizes
    assert sum(1 for c in CASES if c[0].startswith("random")) >= 20


def test_avoid_set_drops_the_symmetries_that_do_not_preserve_it():
    # the centre's N move: the flips keep it, the transposes turn it into the W move
    e, r = run(5, 5, 4, [], avoid=[0 * 25 + 12])
    assert e["root"] == list(range(8)) and r["symmetries"] == e["used"] == [0, 1, 2, 3]
    check(e, r)
    assert r["mask"][12]
    # an asymmetric avoid set leaves the identity: nothing but the set is masked
    e, r = run(5, 5, 4, [], avoid=[1])
    assert r["symmetries"] == [0] and r["mask"].sum() == 1 and r["left"] == 95
    check(e, r)
    # allow is the complement of its list
    e, r = run(5, 5, 4, [], allow=[12, 25 + 12, 3])
    check(e, r)
    assert set(np.nonzero(~r["mask"])[0]) <= {12, 25 + 12, 3}


def test_allow_list_of_illegal_moves_is_the_empty_set_signal():
    moves = [0 * 25 + 12]
    e, r = run(5, 5, 4, moves, allow=[12, 25 + 12])  # the occupied cell
    assert r["left"] == 0 and r["num_masked"] == int(e["legal"].sum())
    e, r = run(5, 5, 4, moves, avoid=list(np.nonzero(e["legal"])[0]))
    assert r["left"] == 0
    # pruning alone never empties the set
    for _, X, Y, W, mv in CASES:
        assert run(X, Y, W, mv)[1]["left"] >= 1


def test_bits_past_p_and_bad_modes_are_rejected():
    e = rc.expected(5, 5, 4, [])
    col, hc, hd = rc.library_inputs(e["board"], e["hist"])
    bits = np.zeros(kc.ANALYSIS_RESTRICT_WORDS, np.uint32)
    bits[3] = 1 << 4  # position 100 on a board of 100
    for mode in (1, 2):
        with pytest.raises(kc.CoffeeError, match="position >= 100"):
            kc.root_mask(5, 5, 4, col, hc, hd, e["legal"], avoid_bits=bits, mode=mode)
    kc.root_mask(5, 5, 4, col, hc, hd, e["legal"], avoid_bits=bits, mode=0)  # ignored without a mode
    with pytest.raises(kc.CoffeeError, match="mode"):
        kc.root_mask(5, 5, 4, col, hc, hd, e["legal"], avoid_bits=np.zeros(11, np.uint32), mode=3)
    with pytest.raises(kc.CoffeeError):
        kc.root_mask(5, 5, 4, col, hc, hd, e["legal"], avoid_moves=[1], allow_moves=[2])
    # a board whose positions do not fit the query's words takes pruning but no set
    e = rc.expected(10, 10, 5, [])
    col, hc, hd = rc.library_inputs(e["board"], e["hist"])
    r = kc.root_mask(10, 10, 5, col, hc, hd, e["legal"])
    np.testing.assert_array_equal(r["mask"], e["mask"])
    with pytest.raises(kc.CoffeeError, match="at most 352"):
        kc.root_mask(10, 10, 5, col, hc, hd, e["legal"], avoid_moves=[1])
