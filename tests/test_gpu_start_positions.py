"""Start positions on the device (coffee_*_set_start_positions): the check
kernel's verdicts, which game starts from which sample (exactly: the host runs the kernel's
own pick), the search from a sample against the analysis engine's search of the same position
(which the oracle pins), the rows and records of such games, off is off, match play, the CLI.

Everything is 5x5/4 with the stand-in network, NN cache off, 24 visits and node_cap 128
unless stated."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("coffee_rules", os.path.join(REPO, "tests", "helpers",
                                                                            "coffee_rules.py"))
cr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cr)

SEED, VISITS, CAP = 11, 24, 128
X, Y, W, A = 5, 5, 4, 25


def _engine(games, **kw):
    kw.setdefault("seed", SEED)
    return kc.Selfplay(X, Y, W, num_games=games, max_visits=VISITS, node_cap=CAP, commit_interval=1, **kw)


def _table(lengths, seed=5, x=X, y=Y, w=W):
    rng = np.random.default_rng(seed)
    return [cr.random_position(x, y, w, n, rng) for n in lengths]


def _expect_start(moves):
    """(turn, lastCell, lastDir) of game_info after the replay of `moves` (None: empty board)."""
    if not moves:
        return 0, -1, 4
    return len(moves), moves[-1] % A, moves[-1] // A


# ---------------------------------------------------------------------------------------
# 1. The check kernel, and the setter's refusal.

def _check_batch(x, y, w, seed):
    rng = np.random.default_rng(seed)
    a = x * y
    legal6 = cr.random_position(x, y, w, 6, rng)
    bad3 = cr.random_position(x, y, w, 3, rng)
    bad3 = bad3 + [bad3[0]] + cr.random_position(x, y, w, 2, rng)  # index 3: an occupied cell
    over = cr.random_finished_game(x, y, w, rng, a - 1)
    big = cr.random_position(x, y, w, 2, rng) + [4 * a]            # index 2: a move >= P
    return [legal6, [], bad3, over, big]


def test_check_kernel_statuses_5x5():
    batch = _check_batch(X, Y, W, 1)
    status, info = kc.start_positions_check(X, Y, W, batch)
    want = [cr.replay(X, Y, W, m)[:2] for m in batch]
    assert [w[0] for w in want] == [cr.OK, cr.OK, cr.ILLEGAL_MOVE, cr.GAME_OVER, cr.ILLEGAL_MOVE]
    assert want[2][1] == 3 and want[3][1] in (1, 2) and want[4][1] == 2
    assert list(zip(status.tolist(), info.tolist())) == want


def test_check_kernel_statuses_7x7():
    batch = _check_batch(7, 7, 5, 2)  # P = 196: the four-item instance
    status, info = kc.start_positions_check(7, 7, 5, batch)
    assert list(zip(status.tolist(), info.tolist())) == [cr.replay(7, 7, 5, m)[:2] for m in batch]


def test_setter_refuses_a_bad_table_and_leaves_the_engine_alone():
    batch = _check_batch(X, Y, W, 1)
    a, b = _engine(8), _engine(8)
    with pytest.raises(kc.CoffeeError, match="start position 2"):
        a.set_start_positions(batch, 1.0)
    with pytest.raises(kc.CoffeeError):
        a.set_start_positions(batch[:2], 1.5)
    with pytest.raises(kc.CoffeeError):
        a.set_start_positions([(batch[0], -1.0)], 1.0)
    assert a.start_position_games() == 0
    a.step(60)
    b.step(60)
    for g in range(8):
        assert a.game_info(g) == b.game_info(g)
        for u, v in zip(a.game_tree(g, CAP), b.game_tree(g, CAP)):
            np.testing.assert_array_equal(u, v)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------
# 2. Who starts where, exactly.

def test_who_starts_where():
    G, prob = 256, 0.5
    lengths = [(3 * i) % 15 for i in range(70)]
    lengths[7] = 0  # one empty-list entry
    moves = _table(lengths)
    weights = [1.0 + (i % 4) for i in range(70)]
    weights[20] = 0.0  # never picked
    table = list(zip(moves, weights))
    lam = 0.1
    cum = kc.start_positions_thresholds(table, lam)
    pick = {(s, n): kc.start_position_pick(SEED, s, n, prob, cum) for s in range(G) for n in range(3)}
    assert 20 not in pick.values() and -1 in pick.values() and 7 in pick.values()
    e = _engine(G)
    e.set_start_positions(table, prob, turn_weight_lambda=lam)
    for s in range(G):
        i = e.game_info(s)
        p = pick[(s, 0)]
        assert (i["turn"], i["lastCell"], i["lastDir"]) == _expect_start(moves[p] if p >= 0 else None), (s, p)
        assert i["gameNum"] == 0 and i["phase"] == 0
    assert e.start_position_games() == sum(1 for s in range(G) if pick[(s, 0)] >= 0)
    # game numbers 1 and 2 from the records (first moves) and the rows (mode, start turn)
    seen, row_seen = {}, {}
    for _ in range(16):
        e.step(250)
        rows = e.drain_rows()
        for m, gt in zip(rows["meta"], rows["globalTargetsNC"]):
            row_seen.setdefault((int(m[0]), int(m[1])), set()).add((int(gt[55]), int(gt[53])))
        hdr, mv = e.drain_games()
        for h, m in zip(hdr, mv):
            seen[(int(h[0]), int(h[1]))] = (int(h[2]), m)
        if all((s, 2) in seen for s in range(G)):
            break
    started = 0
    for s in range(G):
        for n in range(3):
            assert (s, n) in seen, (s, n)
            p = pick[(s, n)]
            num, m = seen[(s, n)]
            want = moves[p] if p >= 0 else []
            assert num >= len(want)
            got = [int(m[t, 1]) * A + int(m[t, 0]) for t in range(len(want))]
            assert got == want, (s, n, p)
            # every row of the game: mode 4 and the sample's length, or mode 0 from the empty board
            assert row_seen.get((s, n), set()) <= {(4, len(want)) if p >= 0 else (0, 0)}, (s, n, p)
    assert sum(len(v) for v in row_seen.values()) > 0
    # the counter: every game started so far (numbers 0 .. the slot's current one)
    for s in range(G):
        for n in range(e.game_info(s)["gameNum"] + 1):
            started += kc.start_position_pick(SEED, s, n, prob, cum) >= 0
    assert e.start_position_games() == started
    assert e.stats()["errors"] == 0
    e.close()


# ---------------------------------------------------------------------------------------
# 3. The search from a sample is the search the analysis engine (and through it the oracle) pins.

def _search_equals_analysis(x, y, w, lengths, games, rounds):
    table = _table(lengths, seed=9, x=x, y=y, w=w)
    cum = kc.start_positions_thresholds(table)
    sp = kc.Selfplay(x, y, w, num_games=games, max_visits=VISITS, node_cap=CAP, commit_interval=1, seed=SEED)
    sp.set_start_positions(table, 1.0)
    ans = []
    for s in range(games):
        p = kc.start_position_pick(SEED, s, 0, 1.0, cum)
        assert p >= 0
        an = kc.Analysis(x, y, w, num_slots=1, seed=SEED, node_cap=CAP, query_capacity=4,
                         search=kc.default_search_params(max_visits=VISITS))
        assert an.submit([dict(id=s + 1, moves=table[p], max_visits=VISITS, stream=s, game_num=0,
                               rng_counter=sp.game_info(s)["rngCtr"])]) == 1
        ans.append(an)
    picks = {kc.start_position_pick(SEED, s, 0, 1.0, cum) for s in range(games)}
    for r in range(rounds):
        sp.step(1)
        for s, an in enumerate(ans):
            an.step(1)
            for u, v in zip(sp.game_tree(s, CAP), an.game_tree(0, CAP)):
                np.testing.assert_array_equal(u, v, err_msg="slot %d round %d" % (s, r))
            gi, ai = sp.game_info(s), an.game_info(0)
            for k in ("phase", "rootK", "liveCount", "turn", "pla", "lastCell", "lastDir", "rngCtr"):
                assert gi[k] == ai[k], (s, r, k)
            if gi["phase"] == 1:
                np.testing.assert_array_equal(sp.root_policy(s), an.root_policy(0))
    assert sp.game_tree(0, CAP)[0][0, 0] >= rounds // 2  # the searches did run
    for an in ans:
        an.close()
    sp.close()
    return picks


def test_search_from_a_sample_equals_analysis_5x5():
    picks = _search_equals_analysis(X, Y, W, [0, 5, 12], 8, 20)
    assert len(picks) >= 2


def test_search_from_a_sample_equals_analysis_7x7():
    _search_equals_analysis(7, 7, 5, [9], 2, 20)


# ---------------------------------------------------------------------------------------
# 4. Rows and records.

def _play_out(e, G, want_games):
    rows, recs = [], []
    for _ in range(20):
        e.step(250)
        r = e.drain_rows()
        rows.append(r)
        hdr, mv = e.drain_games()
        recs += [(int(h[0]), int(h[1]), int(h[2]), m) for h, m in zip(hdr, mv)]
        if len({(s, n) for s, n, _, _ in recs if n == 0}) >= want_games:
            break
    cat = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    return cat, recs


M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _init_moves(seed, slot, game, prop):
    """startGame's policy-init count of a game that took a sample at prob 1 (draws 1-2 the game
    hashes, 3-4 the pick, from 5 on the first u > 0): floor(-log(u) * (A * prop)) in float32."""
    if prop <= 0.0:
        return 0
    st = _mix64(seed ^ _mix64((slot << 32) | game))
    ctr, u = 5, np.float32(0.0)
    while True:
        u = np.float32(_mix64(st ^ ((ctr * 0xd1342543de82ef95) & M64)) >> 40) * np.float32(1.0 / 16777216.0)
        if u > 0:
            break
        ctr += 1
    return int(np.floor(np.float32(-np.log(u)) * (np.float32(A) * np.float32(prop))))


def _check_games(rows, recs, table, cum, init_prop):
    """Every finished game: the record begins with the picked sample; gt[53] is the sample's length
    plus the policy-init moves (restated from the game's stream); the game's own rows (gt[27] == 1;
    side-position rows have 0) are exactly one per turn from there to the end, none below; planes
    0-2 of the first row are the board after the record's first gt[53] moves.  Returns how many
    games had policy-init moves on top of their sample."""
    meta, gt, binp = rows["meta"], rows["globalTargetsNC"], rows["binaryInputNCHWPacked"]
    assert len(meta) > 0 and np.all(gt[:, 55] == 4)
    own = gt[:, 27] == 1
    longer = checked = 0
    for s, n, num, m in recs:
        want = table[kc.start_position_pick(SEED, s, n, 1.0, cum)]
        moves = [int(m[t, 1]) * A + int(m[t, 0]) for t in range(num)]
        assert moves[:len(want)] == want, (s, n)
        sel = (meta[:, 0] == s) & (meta[:, 1] == n)
        start = len(want) + _init_moves(SEED, s, n, init_prop)
        if not (sel & own).any():
            assert start >= num, (s, n, start, num)  # the game ended within its unsearched moves
            continue
        assert np.all(gt[sel, 53] == start), (s, n, start, gt[sel, 53])
        assert sorted(meta[sel & own, 2].tolist()) == list(range(start, num)), (s, n, start, num)
        assert np.all(meta[sel & own, 3] == num) and meta[sel, 2].min() >= start
        first = np.nonzero(sel & own & (meta[:, 2] == start))[0]
        _, _, b = cr.replay(X, Y, W, moves[:start])
        np.testing.assert_array_equal(np.unpackbits(binp[first[0]], axis=1)[:3, :A], cr.planes012(b))
        longer += start > len(want)
        checked += 1
    assert checked > 0
    return longer


@pytest.mark.parametrize("init_prop", [0.0, 0.2])
def test_rows_and_records(init_prop):
    G = 16
    table = _table([2, 6, 11], seed=3)
    cum = kc.start_positions_thresholds(table)
    e = _engine(G, init_games_with_policy=1, policy_init_area_prop=0.0, policy_init_area_temperature=1.0)
    e.set_start_positions(table, 1.0, start_policy_init_area_prop=init_prop)
    rows, recs = _play_out(e, G, G)
    longer = _check_games(rows, recs, table, cum, init_prop)
    assert len(recs) >= G and (longer > 0) == (init_prop > 0.0)
    assert e.stats()["errors"] == 0
    e.close()


@pytest.mark.parametrize("init_prop", [0.0, 0.2])
def test_side_positions_on_top_of_start_positions(init_prop):
    """With side positions on, a slot's next game can start from sideEval (a round kernel) instead
    of the commit: its sample's turn records must be there all the same."""
    G = 32
    table = _table([2, 6, 11], seed=3)
    cum = kc.start_positions_thresholds(table)
    e = _engine(G, init_games_with_policy=1, policy_init_area_prop=0.0, policy_init_area_temperature=1.0,
                side_position_prob=0.3)
    e.set_start_positions(table, 1.0, start_policy_init_area_prop=init_prop)
    rows, recs = [], []
    for _ in range(12):
        e.step(250)
        rows.append(e.drain_rows())
        hdr, mv = e.drain_games()
        recs += [(int(h[0]), int(h[1]), int(h[2]), m) for h, m in zip(hdr, mv)]
    rows = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    # only games whose rows and side rows are all out: not a slot's newest record
    last = {}
    for s, n, _, _ in recs:
        last[s] = max(last.get(s, -1), n)
    done = [r for r in recs if r[1] < last[r[0]]]
    assert len(done) >= 2 * G
    assert np.count_nonzero(rows["globalTargetsNC"][:, 27] == 0) > G  # side-position rows were written
    longer = _check_games(rows, done, table, cum, init_prop)
    assert (longer > 0) == (init_prop > 0.0)
    st = e.stats()
    assert st["errors"] == 0 and e.start_position_games() >= len(recs)
    e.close()


def test_forks_on_top_of_start_positions():
    G = 32
    table = _table([2, 6, 11], seed=3)
    e = _engine(G, early_fork_game_prob=0.3, early_fork_game_expected_move_prop=0.2, fork_game_prob=0.2,
                fork_game_min_choices=2, early_fork_game_max_choices=4, fork_game_max_choices=4)
    e.set_start_positions(table, 0.5)
    modes = set()
    for _ in range(8):
        e.step(250)
        modes |= set(e.drain_rows()["globalTargetsNC"][:, 55].astype(int).tolist())
        e.drain_games()
    st = e.stats()
    assert st["errors"] == 0 and st["games_finished"] > G
    assert modes == {0, 2, 4}
    e.close()


# ---------------------------------------------------------------------------------------
# 5. Off is off.

def test_off_is_off():
    G = 64
    table = _table([2, 6, 11], seed=3)
    engines = [_engine(G) for _ in range(3)]
    engines[0].set_start_positions(table, 0.0)
    engines[1].set_start_positions([], 1.0)
    for e in engines:
        e.step(90)
    assert min(engines[2].game_info(g)["moves"] for g in range(G)) >= 3
    for g in range(G):
        ref = engines[2].game_tree(g, CAP)
        for e in engines[:2]:
            assert e.game_info(g) == engines[2].game_info(g)
            for u, v in zip(e.game_tree(g, CAP), ref):
                np.testing.assert_array_equal(u, v)
    for e in engines:
        e.step(700)
    def row_set(e):
        # the rows of one commit land in the buffer in the order their games reserved them,
        # which is not fixed: compared as sorted whole rows
        r = e.drain_rows()
        n = len(r["meta"])
        return sorted(b"".join(np.ascontiguousarray(r[k][i]).tobytes() for k in sorted(r)) for i in range(n))

    ref = row_set(engines[2])
    assert len(ref) > 0
    for e in engines[:2]:
        assert row_set(e) == ref
        assert e.start_position_games() == 0
    for e in engines:
        e.close()


# ---------------------------------------------------------------------------------------
# 6. Match play.

def _match(G):
    return kc.Match(X, Y, W, num_games=G, seed=SEED, node_cap=CAP, commit_interval=1, max_visits=VISITS)


def _match_records(m, rounds):
    recs = []
    for _ in range(rounds // 250):
        m.step(250)
        hdr, mv = m.drain_games()
        recs += [(h.tolist(), x) for h, x in zip(hdr, mv)]
    return recs


def test_match_games_start_from_samples():
    G = 16
    table = _table([1, 4, 8], seed=4)
    cum = kc.start_positions_thresholds(table)
    m = _match(G)
    m.set_start_positions(table, 1.0)
    for s in range(G):
        i = m.game_info(s)
        assert (i["turn"], i["lastCell"], i["lastDir"]) == _expect_start(table[kc.start_position_pick(SEED, s, 0, 1.0,
                                                                                                      cum)])
    recs = _match_records(m, 1500)
    assert len(recs) >= G
    for (s, n, num, winner, cand), mv in recs:
        want = table[kc.start_position_pick(SEED, s, n, 1.0, cum)]
        assert [int(mv[t, 1]) * A + int(mv[t, 0]) for t in range(len(want))] == want
        assert cand == (1 if (s + n) % 2 == 0 else 2)
    assert m.stats()["errors"] == 0
    m.close()


def test_match_setter_mid_run_applies_to_later_games():
    G = 16
    table = _table([3, 4, 8], seed=4)
    cum = kc.start_positions_thresholds(table)
    m, ref = _match(G), _match(G)
    m.step(100)
    ref.step(100)
    m.set_start_positions(table, 1.0)
    assert m.start_position_games() == 0
    for s in range(G):  # the games in progress are untouched
        assert m.game_info(s) == ref.game_info(s)
    ref.close()
    recs = _match_records(m, 1500)
    later = 0
    for (s, n, num, winner, cand), mv in recs:
        if n == 0:
            continue
        later += 1
        want = table[kc.start_position_pick(SEED, s, n, 1.0, cum)]
        assert [int(mv[t, 1]) * A + int(mv[t, 0]) for t in range(len(want))] == want
    assert later > 0 and m.start_position_games() >= later
    m.close()


# ---------------------------------------------------------------------------------------
# 7. The command: `katago selfplay` starts games from the .sgfs files an earlier run wrote.

def test_cli_selfplay_reads_its_own_sgfs(tmp_path):
    import glob
    import re
    models = tmp_path / "models"
    models.mkdir()
    kc.write_random_model("b6c96", 5, str(models / "b6c96-s0.cfnn"))
    katago = os.path.join(REPO, "katacoffee_amd", "katago")
    base = [katago, "selfplay", "-config", os.path.join(REPO, "configs", "selfplay_coffee5.cfg"), "-models-dir",
            str(models), "-max-games-total", "24", "-override-config"]
    over = "numGameThreads=32,maxVisits=8,maxRowsPerTrainFile=100"
    first = tmp_path / "first"
    r = subprocess.run(base[:6] + ["-output-dir", str(first)] + base[6:] + [over], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    sgfs = first / "b6c96-s0" / "sgfs"
    assert glob.glob(str(sgfs / "*.sgfs"))
    second = tmp_path / "second"
    r = subprocess.run(base[:6] + ["-output-dir", str(second)] + base[6:] +
                       [over + ",startPosesFromSgfDir=%s,startPosesProb=1,startPosesLoadProb=0.5,"
                        "initGamesWithPolicy=false" % sgfs], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    m = re.search(r"start positions: \d+ files, (\d+) games, (\d+) candidates; kept (\d+),", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 24 and 0 < int(m.group(3)) < int(m.group(2))
    assert "effective sample size" in r.stdout
    files = glob.glob(str(second / "b6c96-s0" / "tdata" / "*.npz"))
    assert files, r.stdout
    for f in files:
        with np.load(f) as z:
            np.testing.assert_array_equal(z["globalTargetsNC"][:, 55], 4.0)
            assert z["globalTargetsNC"][:, 53].min() >= 1  # every sample has at least one move
