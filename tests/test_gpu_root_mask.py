"""Root move restrictions of analysis on the device: the root symmetries are
the ones the encoder cannot see, the device's mask is the host rule's, the search never
expands a masked move and is otherwise untouched, avoid / allow sets and the empty-set answer,
and what pruning buys on the empty 5x5 board.

Stand-in network and 64-visit queries unless stated; 5x5/4 (two items per lane), 7x7/5 (four)
and 9x9/5 (seven)."""
import importlib.util
import os

import numpy as np
import pytest

import katacoffee_amd as kc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("root_mask_cases",
                                               os.path.join(REPO, "tests", "helpers", "root_mask_cases.py"))
rc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rc)

CASES = rc.cases()
VISITS, CAP = 64, 256
GEOMS = [(5, 5, 4), (7, 7, 5), (9, 9, 5)]


def host_rule(X, Y, W, moves, avoid=None, allow=None, prune=True):
    e = rc.expected(X, Y, W, moves, avoid=avoid, allow=allow, prune=prune)
    col, hc, hd = rc.library_inputs(e["board"], e["hist"])
    return e, kc.root_mask(X, Y, W, col, hc, hd, e["legal"], avoid_moves=avoid, allow_moves=allow, prune=prune)


def engine(X, Y, W, slots=1, **kw):
    return kc.Analysis(X, Y, W, num_slots=slots, seed=23, node_cap=CAP, query_capacity=64, max_visits=VISITS, **kw)


def one(X, Y, W, query, **kw):
    """One query through a one-slot engine: its result and the tree and noised root policy the
    idle slot keeps."""
    an = engine(X, Y, W, **kw)
    h, m, root, pol = an.analyze([query], with_root=True)
    nodes, edges = an.game_tree(0)
    rp = an.root_policy(0)
    st = an.stats()
    an.close()
    assert st["errors"] == 0
    k = int(h[0]["num_children"])
    return dict(h=h[0], m=m[0][:k], raw=(h.tobytes(), m.tobytes()), root=root[0], policy=None if pol is None else pol[0],
                nodes=nodes, edges=edges, root_policy=rp, k=k)


def children_of(r):
    k = int(r["nodes"][0, 10] & 0xFFFF)
    assert k == r["k"]
    return [int(x) for x in r["edges"][0, :k, 2]]


# ---------------------------------------------------------------------------------------
# 1. The definition's witness: the encoder and the rules cannot tell the root symmetries apart.

@pytest.mark.parametrize("X,Y,W", GEOMS + [(6, 4, 3)])
def test_encoder_and_rules_witness_the_root_symmetries(X, Y, W):
    A, P = X * Y, 4 * X * Y
    cases = [c for c in CASES if (c[1], c[2], c[3]) == (X, Y, W)]
    assert cases
    n = len(cases)
    cells = np.zeros((8 * n, A), np.uint8)
    hc = np.full((8 * n, 5), -1, np.int8)
    hd = np.full((8 * n, 5), 4, np.int8)
    pla = np.zeros(8 * n, np.uint8)
    want = []
    for i, (_, _, _, _, moves) in enumerate(cases):
        e, r = host_rule(X, Y, W, moves)
        want.append((e, r))
        for s in range(8):
            cells[8 * i + s] = e["board"].cells
            for k, (c, d) in enumerate(e["hist"]):
                hc[8 * i + s, k], hd[8 * i + s, k] = c, d
            pla[8 * i + s] = e["board"].pla
    sym = np.tile(np.arange(8), n).astype(np.int32)
    packed, _ = kc.encode_batch(X, Y, W, cells, hc, hd, pla, sym, want_planes=False)
    legal, _ = kc.rules_batch(X, Y, W, cells[::8], hc[::8, 0].copy(), hd[::8, 0].copy(), pla[::8])
    for i, (e, r) in enumerate(want):
        group = range(8) if X == Y else range(4)
        same = [s for s in group if np.array_equal(packed[8 * i + s], packed[8 * i])]
        assert same == r["symmetries"] == e["root"], cases[i][0]
        lg = legal[i].astype(bool)
        np.testing.assert_array_equal(lg, e["legal"])
        for s in same:
            img = np.array([kc.symmetry_move(X, Y, s, p) for p in range(P)])
            np.testing.assert_array_equal(lg[img], lg)


# ---------------------------------------------------------------------------------------
# 2. The device's mask is the host rule's.

@pytest.mark.parametrize("X,Y,W", GEOMS)
def test_device_symmetries_and_masked_counts_equal_the_host_rule(X, Y, W):
    cases = [c for c in CASES if (c[1], c[2], c[3]) == (X, Y, W)]
    queries, want = [], []
    for i, (_, _, _, _, moves) in enumerate(cases):
        for kw in ({}, {"avoid": [0, 7]}, {"allow": [1, 2, 2 * X * Y + X + 1, 3 * X * Y + 2 * X + 1, X * Y + 3]}):
            e, r = host_rule(X, Y, W, moves, **kw)
            q = dict(id=len(queries) + 1, moves=moves, max_visits=8)
            if "avoid" in kw:
                q["avoid_moves"] = kw["avoid"]
            if "allow" in kw:
                q["allow_moves"] = kw["allow"]
            queries.append(q)
            want.append(r)
    an = engine(X, Y, W, slots=8, root_symmetry_pruning=True)
    h, m, root, _ = an.analyze(queries, with_root=True)
    assert an.stats()["errors"] == 0
    an.close()
    searched = 0
    for i, r in enumerate(want):
        assert h[i]["status"] == (kc.ANALYSIS_OK if r["left"] > 0 else kc.ANALYSIS_NO_ALLOWED_MOVE), i
        assert root[i]["symmetries"] == r["bits"] and root[i]["num_masked"] == r["num_masked"], (i, queries[i])
        k = int(h[i]["num_children"])
        assert not r["mask"][m[i]["move"][:k]].any()
        searched += h[i]["status"] == kc.ANALYSIS_OK
    assert searched > len(cases)


# ---------------------------------------------------------------------------------------
# 3. The search obeys the mask and is otherwise the unrestricted search's.

@pytest.mark.parametrize("X,Y,W,moves", [(5, 5, 4, []), (5, 5, 4, [12]), (7, 7, 5, [2 * 49 + 24]), (9, 9, 5, [])])
def test_search_obeys_the_mask(X, Y, W, moves):
    P = 4 * X * Y
    e, r = host_rule(X, Y, W, moves)
    assert len(r["symmetries"]) > 1
    q = dict(id=5, moves=moves)
    a = one(X, Y, W, q, root_symmetry_pruning=True, include_policy=True)
    b = one(X, Y, W, q, include_policy=True)
    assert a["h"]["status"] == kc.ANALYSIS_OK and a["h"]["visits"] == VISITS == a["nodes"][0, 0]
    assert a["root"]["symmetries"] == r["bits"] and a["root"]["num_masked"] == r["num_masked"] > 0
    assert b["root"]["symmetries"] == r["bits"] and b["root"]["num_masked"] == 0
    kids = children_of(a)
    assert kids == [int(x) for x in a["m"]["move"]] and kids
    assert not r["mask"][kids].any()
    # prior and policy: the unmasked values
    np.testing.assert_array_equal(a["policy"].view(np.uint32), b["policy"].view(np.uint32))
    np.testing.assert_array_equal(a["policy"] >= 0, e["legal"])
    np.testing.assert_array_equal(a["m"]["prior"].view(np.uint32), a["policy"][kids].view(np.uint32))
    prior_b = {int(mv): p for mv, p in zip(b["m"]["move"], b["m"]["prior"].view(np.uint32))}
    for mv, p in zip(kids, a["m"]["prior"].view(np.uint32)):
        if mv in prior_b:
            assert p == prior_b[mv]
    # the noised root policy: -1 exactly at illegal or masked positions, else the unrestricted run's
    gone = r["mask"] | ~e["legal"]
    assert np.all(a["root_policy"][gone] == -1.0) and np.all(a["root_policy"][~gone] >= 0.0)
    np.testing.assert_array_equal(a["root_policy"][~gone].view(np.uint32), b["root_policy"][~gone].view(np.uint32))
    assert len(a["root_policy"]) == P


# ---------------------------------------------------------------------------------------
# 4. No mask, no change.

def test_trivial_group_without_a_set_changes_nothing():
    trivial = [c for c in CASES if c[0].startswith("random") and (c[1], c[2]) == (5, 5)
               and len(rc.expected(c[1], c[2], c[3], c[4])["used"]) == 1]
    assert trivial
    _, X, Y, W, moves = trivial[0]
    q = dict(id=9, moves=moves)
    a = one(X, Y, W, q, root_symmetry_pruning=True)
    b = one(X, Y, W, q)
    assert a["raw"] == b["raw"] and a["root"]["symmetries"] == 1 and a["root"]["num_masked"] == 0
    np.testing.assert_array_equal(a["nodes"], b["nodes"])
    np.testing.assert_array_equal(a["edges"], b["edges"])
    np.testing.assert_array_equal(a["root_policy"].view(np.uint32), b["root_policy"].view(np.uint32))


def test_submit2_and_drain2_with_the_options_off_equal_submit_and_drain():
    queries = [dict(id=i + 1, moves=c[4]) for i, c in enumerate(CASES) if (c[1], c[2]) == (5, 5)][:8]
    out = []
    for two in (False, True):
        an = engine(5, 5, 4, slots=4)
        assert (an.submit2(queries) if two else an.submit(queries)) == len(queries)
        got = []
        for _ in range(200):
            an.step(16)
            res = an.drain2() if two else an.drain()
            got += [(res[0][i].tobytes(), res[1][i].tobytes()) for i in range(len(res[0]))]
            if len(got) == len(queries):
                break
        an.close()
        out.append(sorted(got))  # (completion order depends on which slot reports first)
    assert len(out[0]) == len(queries) and out[0] == out[1]


# ---------------------------------------------------------------------------------------
# 5. Avoid and allow.

def test_avoid_and_allow_sets():
    moves = [c for c in CASES if c[0] == "random0"][0][4]
    e, _ = host_rule(5, 5, 4, moves)
    free = one(5, 5, 4, dict(id=1, moves=moves))
    best = int(free["m"]["move"][np.argmax(free["m"]["edge_visits"])])
    av = one(5, 5, 4, dict(id=1, moves=moves, avoid_moves=[best]))
    assert av["h"]["status"] == kc.ANALYSIS_OK and av["h"]["visits"] == VISITS
    assert best not in children_of(av) and children_of(av) and av["root"]["num_masked"] == 1
    assert av["root_policy"][best] == -1.0
    two = [int(x) for x in np.nonzero(e["legal"])[0][[0, -1]]]
    al = one(5, 5, 4, dict(id=1, moves=moves, allow_moves=two))
    assert al["h"]["visits"] == VISITS and 1 <= len(children_of(al)) <= 2 and set(children_of(al)) <= set(two)
    assert al["root"]["num_masked"] == int(e["legal"].sum()) - 2


def test_an_allow_list_without_a_legal_move_is_answered_without_a_search():
    moves = [12]
    an = engine(5, 5, 4)
    assert an.submit([dict(id=1, moves=moves, allow_moves=[12, 25 + 12]), dict(id=2, moves=moves)]) == 2
    an.step(0)  # the load alone: the first query is answered, the slot holds the second
    h, m, root, _ = an.drain(with_root=True)
    st = an.stats()
    assert len(h) == 1 and h[0]["id"] == 1 and h[0]["status"] == kc.ANALYSIS_NO_ALLOWED_MOVE
    assert h[0]["visits"] == 0 and h[0]["num_children"] == 0 and h[0]["turn"] == 1 and h[0]["pla"] == 2
    e, r = host_rule(5, 5, 4, moves, allow=[12, 25 + 12])
    assert root[0]["num_masked"] == int(e["legal"].sum()) and root[0]["symmetries"] == r["bits"]
    assert st["queries_rejected"] == 1 and st["queries_loaded"] == 2 and st["playouts"] == 0 and st["errors"] == 0
    assert an.game_info(0)["turn"] == 1 and an.game_info(0)["phase"] == 0
    assert an.submit([dict(id=3, moves=moves)]) == 1  # the second finishes, then a third
    done = {}
    for _ in range(100):
        an.step(16)
        h, _ = an.drain()
        done.update({int(x["id"]): int(x["status"]) for x in h})
        if len(done) == 2:
            break
    st = an.stats()
    an.close()
    assert done == {2: kc.ANALYSIS_OK, 3: kc.ANALYSIS_OK} and st["queries_finished"] == 3 and st["errors"] == 0


@pytest.mark.parametrize("pruning", [False, True])
def test_answers_without_a_search_in_one_load_keep_their_statuses(pruning):
    # statuses 1, 1, 2, 1 and 4 answered back to back by one slot in one launch, then a search
    won = rc.rules.random_finished_game(5, 5, 4, np.random.default_rng(3), 25)
    b = rc.rules.Board(5, 5, 4)
    b.play(won[0])
    occupied = [won[0], won[0]]
    off_line = [won[0], next(p for p in range(100) if b.cells[p % 25] == 0 and not b.legal(p % 25, p // 25))]
    an = engine(5, 5, 4, root_symmetry_pruning=pruning)
    qs = [dict(id=1, moves=occupied), dict(id=2, moves=off_line), dict(id=3, moves=won),
          dict(id=4, moves=won + [won[0]]), dict(id=5, moves=[12], allow_moves=[12]), dict(id=6, moves=won[:-1])]
    assert an.submit(qs) == 6
    an.step(0)
    h, _, root, _ = an.drain(with_root=True)
    print("moves", won, "results", [(int(x["id"]), int(x["status"]), int(x["info"]), int(x["turn"])) for x in h])
    assert [int(x) for x in h["id"]] == [1, 2, 3, 4, 5]
    assert [int(x) for x in h["status"]] == [1, 1, 2, 1, 4]
    assert [int(x) for x in h["info"][:4]] == [1, 1, 1 + (len(won) - 1) % 2, len(won)]
    assert np.all(root["symmetries"][:4] == 0) and np.all(root["num_masked"][:4] == 0)
    h, _ = an.analyze([dict(id=7, moves=[])])
    st = an.stats()
    an.close()
    assert st["queries_finished"] == 7 and st["queries_rejected"] == 5 and st["errors"] == 0


def test_bad_restrictions_and_late_options_are_rejected():
    an = engine(5, 5, 4)
    bad = np.zeros(1, kc.ANALYSIS_RESTRICT)
    bad[0]["avoid"][3] = 1 << 4
    bad[0]["mode"] = 1
    with pytest.raises(kc.CoffeeError, match="position >= 100"):
        an.submit2([dict(id=1, moves=[])], bad)
    with pytest.raises(kc.CoffeeError, match="exclusive"):
        an.submit([dict(id=1, moves=[], avoid_moves=[1], allow_moves=[2])])
    assert an.stats()["queries_loaded"] == 0
    with pytest.raises(kc.CoffeeError, match="include_policy"):
        kc.check(kc.lib().coffee_analysis_drain2(an.h, 1, None, None, None, kc._ptr(np.zeros(100, np.float32)),
                                                 kc.ctypes.byref(kc.ctypes.c_int())))
    assert an.submit([dict(id=1, moves=[])]) == 1
    with pytest.raises(kc.CoffeeError, match="before the first query"):
        an.set_root_options(True, False)
    an.close()


# ---------------------------------------------------------------------------------------
# 6. What pruning buys on the empty 5x5 board.

def test_empty_board_pruning_concentrates_the_visits():
    e, r = host_rule(5, 5, 4, [])
    q = dict(id=4, moves=[])
    a = one(5, 5, 4, q, root_symmetry_pruning=True)
    b = one(5, 5, 4, q)
    survivors = set(np.nonzero(e["legal"] & ~r["mask"])[0].tolist())
    assert set(children_of(a)) <= survivors and len(survivors) == 17
    top_a, top_b = int(a["m"]["edge_visits"].max()), int(b["m"]["edge_visits"].max())
    print("empty 5x5, %d visits: most-visited child %d edge visits of %d children pruned, %d of %d unpruned"
          % (VISITS, top_a, a["k"], top_b, b["k"]))
    assert top_a > top_b


# ---------------------------------------------------------------------------------------
# 7. A real network: rareLeaf's network-fed root path.

def test_pruning_with_a_network(tmp_path):
    path = str(tmp_path / "b6c96.cfnn")
    kc.write_random_model("b6c96", 3, path)
    e, r = host_rule(5, 5, 4, [12])
    q = dict(id=6, moves=[12], max_visits=32)
    a = one(5, 5, 4, q, model_path=path, root_symmetry_pruning=True, include_policy=True)
    b = one(5, 5, 4, q, model_path=path, include_policy=True)
    assert a["h"]["status"] == kc.ANALYSIS_OK and a["h"]["visits"] == 32
    assert a["root"]["symmetries"] == r["bits"] and a["root"]["num_masked"] == r["num_masked"] > 0
    assert children_of(a) and not r["mask"][children_of(a)].any()
    np.testing.assert_array_equal(a["policy"].view(np.uint32), b["policy"].view(np.uint32))
    gone = r["mask"] | ~e["legal"]
    assert np.all(a["root_policy"][gone] == -1.0)
    np.testing.assert_array_equal(a["root_policy"][~gone].view(np.uint32), b["root_policy"][~gone].view(np.uint32))
