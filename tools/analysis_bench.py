#!/usr/bin/env python3
"""Analysis throughput beside self-play at the same settings (DESIGN.md "Analysis").

  python tools/analysis_bench.py [--arch b6c96] [--slots 4096] [--visits 500] [--rounds 2000]
                                 [--warmup 1000] [--precision default] [--repeats 3]
                                 [--root-symmetry-pruning]
  python tools/analysis_bench.py --queries 1 --slots 1 --visits 1600 --search-threads 1,16 [--step 4]

A kc.Analysis engine is kept fed with queries (random legal openings of 0..8 moves, made with
the device rules) so that its ring never runs dry; a kc.Selfplay engine with the same net,
slots, visits, search parameters, commit interval and cache runs the same rounds for
comparison.  Each figure is taken over `repeats` timed windows of `rounds` rounds after
`warmup` rounds, host clock around work that ends in a device synchronise; submissions and
drains happen between the windows' steps and are part of the analysis time, as they are for a
service.  Prints one JSON line.  The round kernels are the same in both engines, so the
playouts per second should agree; a gap means idle slots or a refill stall.
--root-symmetry-pruning turns the analysis engine's root symmetry pruning on;
with or without it the line also carries the drained results' mean root children and mean
principal-variation length and, where the library reports them, the share of results whose
used symmetry group was not trivial.

--queries N is the latency mode: N queries are submitted at once to an engine of
--slots slots and the time to the last answer is taken, `repeats` times on fresh positions after
one untimed set, for each value of --search-threads (parallel playouts per search,
set_search_threads) in turn, each on an engine of its own (an empty NN cache) and on the same
positions.  One JSON line per value: seconds to the last
answer, playouts per second, collisions per descent, mean root children and mean principal-
variation length.  A library without the setting (an earlier build run as an A/B reference
through KATACOFFEE_LIB) takes --search-threads 1 only."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import katacoffee_amd as kc  # noqa: E402

X, Y, W, A = 5, 5, 4, 25


def openings(n, max_moves, seed):
    """n random legal move lists of 0..max_moves moves that do not end the game."""
    rng = np.random.default_rng(seed)
    cells = np.zeros((n, A), np.uint8)
    lc, ld = np.full(n, -1, np.int8), np.full(n, 4, np.int8)
    pla = np.ones(n, np.uint8)
    want = rng.integers(0, max_moves + 1, n)
    lists = [[] for _ in range(n)]
    for t in range(max_moves):
        on = np.nonzero(want > t)[0]
        if len(on) == 0:
            break
        legal, _ = kc.rules_batch(X, Y, W, cells[on], lc[on], ld[on], pla[on])
        mv = np.array([rng.choice(np.nonzero(row)[0]) for row in legal], np.int32)
        oc, fin, _, _, _, _ = kc.play_batch(X, Y, W, cells[on], lc[on], ld[on], pla[on], mv)
        for j, g in enumerate(on):
            if fin[j]:
                want[g] = t  # keep the position before the move that ends the game
                continue
            lists[g].append(int(mv[j]))
            cells[g], lc[g], ld[g], pla[g] = oc[j], mv[j] % A, mv[j] // A, 3 - pla[g]
    return lists


def latency(a, path, search, pool):
    """The latency mode: time to the last answer of a.queries queries, per --search-threads value.
    Every value gets an engine of its own (an empty NN cache) and the same positions."""
    has = hasattr(kc.lib(), "coffee_virtual_loss")
    for K in [int(k) for k in a.search_threads.split(",")]:
        an = kc.Analysis(X, Y, W, num_slots=a.slots, model_path=path, search=search, seed=7, commit_interval=a.step,
                         query_capacity=max(4 * a.slots, a.queries), nn_cache_log2=a.cache_log2,
                         nn_precision=a.precision)
        next_id = 0
        if has:
            an.set_search_threads(K, a.virtual_losses_per_thread)
        elif K != 1:
            raise SystemExit("this library has no search threads")
        secs, playouts, children, pv, pv_n = [], 0, 0, 0, 0
        i0 = an.search_threads_info() if has else None
        for rep in range(a.repeats + 1):
            qs = [dict(id=next_id + i, moves=pool[(next_id + i) % len(pool)]) for i in range(a.queries)]
            next_id += a.queries
            s0 = an.stats()
            t0 = time.perf_counter()
            assert an.submit(qs) == len(qs)
            got = 0
            while got < len(qs):
                an.step(a.step)
                h, m = an.drain()
                got += len(h)
                if rep > 0 and len(h):
                    assert np.all(h["status"] == 0) and np.all(h["visits"] == a.visits)
                    valid = np.arange(m.shape[1])[None, :] < h["num_children"][:, None]
                    children += int(h["num_children"].sum())
                    pv += int(m["pv_len"][valid].sum())
                    pv_n += int(valid.sum())
            dt = time.perf_counter() - t0
            if rep > 0:  # (the first set is the warm-up)
                secs.append(dt)
                playouts += an.stats()["playouts"] - s0["playouts"]
            elif has:
                i0 = an.search_threads_info()
        i1 = an.search_threads_info() if has else None
        print(json.dumps({
            "mode": "latency", "arch": a.arch, "geometry": [X, Y, W], "slots": a.slots, "queries": a.queries,
            "visits": a.visits, "precision": a.precision, "search_threads": K, "step": a.step,
            "seconds_to_last_answer": [round(x, 5) for x in secs],
            "playouts_per_s": round(playouts / sum(secs), 0),
            "collisions_per_descent": round((i1["collisions"] - i0["collisions"]) /
                                            max(i1["descents"] - i0["descents"], 1), 5) if has and K > 1 else 0.0,
            "mean_root_children": round(children / (a.repeats * a.queries), 2),
            "mean_pv_len": round(pv / max(pv_n, 1), 3)}), flush=True)
        an.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="b6c96")
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--visits", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", type=int, default=100, help="rounds between submissions and drains")
    ap.add_argument("--precision", default="default")
    ap.add_argument("--cache-log2", type=int, default=21)
    ap.add_argument("--uncertainty", action="store_true",
                    help="uncertainty weighting on (set_uncertainty(use_uncertainty=1), default values) in both engines")
    ap.add_argument("--exploration", action="store_true",
                    help="the reference's match / analysis exploration: cpuctUtilityStdevScale 0.85 and noise pruning "
                         "(set_exploration) in both engines")
    ap.add_argument("--root-search", action="store_true",
                    help="wide root noise 0.04 and futile-visit pruning at threshold 0.15 (set_root_search) in both engines")
    ap.add_argument("--root-symmetry-pruning", action="store_true",
                    help="root symmetry pruning on in the analysis engine")
    ap.add_argument("--queries", type=int, default=0,
                    help="latency mode: the time to the last answer of this many queries submitted at once")
    ap.add_argument("--search-threads", default="1",
                    help="latency mode: parallel playouts per search, a comma-separated list measured in turn")
    ap.add_argument("--virtual-losses-per-thread", type=float, default=1.0)
    a = ap.parse_args()
    search = kc.default_analysis_params(max_visits=a.visits)
    pool = openings(8192, 8, 5)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "%s.cfnn" % a.arch)
        kc.write_random_model(a.arch, 1000, path)
        if a.queries > 0:
            latency(a, path, search, pool)
            return
        common = dict(seed=7, commit_interval=16, nn_cache_log2=a.cache_log2, nn_precision=a.precision)
        an = kc.Analysis(X, Y, W, num_slots=a.slots, model_path=path, search=search, query_capacity=4 * a.slots,
                         **common)
        an.set_uncertainty(use_uncertainty=int(a.uncertainty))
        if a.exploration:
            an.set_exploration(**dict(cpuct_utility_stdev_scale=0.85, use_noise_pruning=1))
        if a.root_search:
            an.set_root_search(wide_root_noise=0.04, futile_visits_threshold=0.15)
        has_root = hasattr(kc.lib(), "coffee_root_mask")  # (absent in earlier builds run as A/B references)
        if a.root_symmetry_pruning:
            an.set_root_options(root_symmetry_pruning=True)
        next_id = [0]
        tally = {"results": 0, "children": 0, "pv": 0, "pv_n": 0, "nontrivial": 0}

        def feed():
            free = an.query_capacity - (next_id[0] - feed.drained)
            qs = [dict(id=next_id[0] + i, moves=pool[(next_id[0] + i) % len(pool)]) for i in range(free)]
            next_id[0] += an.submit(qs) if qs else 0

        feed.drained = 0

        def run(rounds):
            done = 0
            while done < rounds:
                feed()
                n = min(a.step, rounds - done)
                an.step(n)
                done += n
                res = an.drain(with_root=True) if has_root else an.drain()
                h, m = res[0], res[1]
                feed.drained += len(h)
                ok = h["status"] == 0
                tally["results"] += int(ok.sum())
                tally["children"] += int(h["num_children"][ok].sum())
                valid = np.arange(m.shape[1])[None, :] < h["num_children"][:, None]
                tally["pv"] += int(m["pv_len"][valid].sum())
                tally["pv_n"] += int(valid.sum())
                if has_root:
                    tally["nontrivial"] += int((res[2]["symmetries"][ok] != 1).sum())

        run(a.warmup)
        an.sync()
        for k in tally:
            tally[k] = 0
        s0, secs = an.stats(), []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            run(a.rounds)
            an.sync()
            secs.append(time.perf_counter() - t0)
        s1 = an.stats()
        an.close()
        t_an = sum(secs)
        over = {k: getattr(search, k) for k, _ in kc.SearchParams._fields_ if k != "max_visits"}
        sp = kc.Selfplay(X, Y, W, num_games=a.slots, model_path=path, max_visits=a.visits, start_stagger=a.visits,
                         **common, **over)
        sp.set_uncertainty(use_uncertainty=int(a.uncertainty))
        if a.exploration:
            sp.set_exploration(**dict(cpuct_utility_stdev_scale=0.85, use_noise_pruning=1))
        if a.root_search:
            sp.set_root_search(wide_root_noise=0.04, futile_visits_threshold=0.15)
        sp.step(a.warmup)
        sp.sync()
        sp.drain_rows()
        sp.drain_games()
        p0, ssecs = sp.stats(), []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            sp.step(a.rounds)
            sp.sync()
            ssecs.append(time.perf_counter() - t0)
            sp.drain_rows()
            sp.drain_games()
        p1 = sp.stats()
        sp.close()
        t_sp = sum(ssecs)
    print(json.dumps({
        "arch": a.arch, "geometry": [X, Y, W], "slots": a.slots, "visits": a.visits, "precision": a.precision,
        "rounds_per_window": a.rounds, "windows": a.repeats, "uncertainty": bool(a.uncertainty),
        "analysis": {"positions_per_s": round((s1["queries_finished"] - s0["queries_finished"]) / t_an, 1),
                     "playouts_per_s": round((s1["playouts"] - s0["playouts"]) / t_an, 0),
                     "us_per_round": round(1e6 * t_an / (a.rounds * a.repeats), 2),
                     "window_s": [round(x, 4) for x in secs],
                     "nn_precision": kc.PRECISION_NAMES.get(s1["nn_precision"], "stand-in"),
                     "root_symmetry_pruning": bool(a.root_symmetry_pruning),
                     "mean_root_children": round(tally["children"] / max(tally["results"], 1), 2),
                     "mean_pv_len": round(tally["pv"] / max(tally["pv_n"], 1), 3),
                     "nontrivial_group_share": round(tally["nontrivial"] / max(tally["results"], 1), 4) if has_root
                     else None},
        "selfplay": {"playouts_per_s": round((p1["playouts"] - p0["playouts"]) / t_sp, 0),
                     "us_per_round": round(1e6 * t_sp / (a.rounds * a.repeats), 2),
                     "window_s": [round(x, 4) for x in ssecs]},
    }))


if __name__ == "__main__":
    main()
