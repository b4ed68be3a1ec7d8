#!/usr/bin/env python3
"""Match-play throughput beside self-play at the same settings (DESIGN.md "Match play").

  python tools/match_bench.py [--arch b6c96] [--games 1024] [--visits 150] [--rounds 3000]
                              [--warmup 600] [--precision default] [--repeats 3]
                              [--equal-sides] [--share-net]

Two seeded random nets of one architecture play each other on one kc.Match engine; a
kc.Selfplay engine with the same net, games, visits, search parameters, commit interval
and cache runs the same number of rounds for comparison.  Each figure is the median of
`repeats` timed windows of `rounds` rounds after `warmup` rounds, host clock around work
that ends in a device synchronise.  Prints one JSON line.  What the comparison says: a
match round runs two network launches (one per net, one after the other) where self-play
runs one, and never fuses backup and select; the difference in time per round is the
price of both, and the bound on what overlapping the two launches could win back.
--equal-sides runs the match with per-side settings, both sides the engine's own (the
per-side code path at unchanged results); --share-net plays one net against itself on one
network instance -- one launch a round, one cache -- which wins the second
launch back."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import katacoffee_amd as kc  # noqa: E402


def timed(engine, rounds, warmup, repeats, drain):
    engine.step(warmup)
    engine.sync()
    drain()
    secs, games0, t_all = [], engine.stats()["games_finished"], 0.0
    for _ in range(repeats):
        t0 = time.perf_counter()
        engine.step(rounds)
        engine.sync()
        secs.append(time.perf_counter() - t0)
        t_all += secs[-1]
        drain()  # outside the window: the records / rows leave the device
    st = engine.stats()
    return secs, (st["games_finished"] - games0) / t_all, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="b6c96")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--visits", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default="default")
    ap.add_argument("--cache-log2", type=int, default=21)
    ap.add_argument("--uncertainty", action="store_true",
                    help="uncertainty weighting on (set_uncertainty(use_uncertainty=1), default values) in both engines")
    ap.add_argument("--exploration", action="store_true",
                    help="the reference's match / analysis exploration: cpuctUtilityStdevScale 0.85 and noise pruning "
                         "(set_exploration) in both engines")
    ap.add_argument("--root-search", action="store_true",
                    help="wide root noise 0.04 and futile-visit pruning at threshold 0.15 (set_root_search) in both engines")
    ap.add_argument("--equal-sides", action="store_true",
                    help="per-side settings with both sides the engine's own parameters (kc.Match(sides=...))")
    ap.add_argument("--share-net", action="store_true",
                    help="one net on both sides, one network instance and launch (kc.Match(share_net=True))")
    a = ap.parse_args()
    X, Y, W = 5, 5, 4
    search = kc.default_match_params(max_visits=a.visits)
    over = {k: getattr(search, k) for k, _ in kc.SearchParams._fields_}
    with tempfile.TemporaryDirectory() as td:
        paths = [os.path.join(td, "%s-%d.cfnn" % (a.arch, i)) for i in range(2)]
        for i, p in enumerate(paths):
            kc.write_random_model(a.arch, 1000 + i, p)
        common = dict(num_games=a.games, seed=7, commit_interval=16, nn_cache_log2=a.cache_log2,
                      nn_precision=a.precision, start_stagger=a.visits)
        extra = {}
        if a.equal_sides:
            unc = kc.default_uncertainty_params(use_uncertainty=int(a.uncertainty))
            extra["sides"] = ((search, unc), (search, unc))
        if a.share_net:
            extra["share_net"] = True
        m = kc.Match(X, Y, W, baseline_path=paths[0], candidate_path=paths[0 if a.share_net else 1], search=search,
                     **common, **extra)
        if not a.equal_sides:  # (the sides carry their own)
            m.set_uncertainty(use_uncertainty=int(a.uncertainty))
        if a.exploration:
            for side in ((0, 1) if a.equal_sides else (-1,)):
                m.set_exploration(side=side, **dict(cpuct_utility_stdev_scale=0.85, use_noise_pruning=1))
        if a.root_search:
            for side in ((0, 1) if a.equal_sides else (-1,)):
                m.set_root_search(side=side, wide_root_noise=0.04, futile_visits_threshold=0.15)
        msecs, mgames, mst = timed(m, a.rounds, a.warmup, a.repeats, m.drain_games)
        m.close()
        over.pop("max_visits")
        s = kc.Selfplay(X, Y, W, model_path=paths[0], max_visits=a.visits, **common, **over)
        s.set_uncertainty(use_uncertainty=int(a.uncertainty))
        if a.exploration:
            s.set_exploration(**dict(cpuct_utility_stdev_scale=0.85, use_noise_pruning=1))
        if a.root_search:
            s.set_root_search(wide_root_noise=0.04, futile_visits_threshold=0.15)

        def drain_sp():
            s.drain_rows()
            s.drain_games()

        ssecs, sgames, sst = timed(s, a.rounds, a.warmup, a.repeats, drain_sp)
        s.close()
    med_m, med_s = statistics.median(msecs), statistics.median(ssecs)
    print(json.dumps({
        "arch": a.arch, "geometry": [X, Y, W], "games": a.games, "visits": a.visits, "precision": a.precision,
        "rounds_per_window": a.rounds, "windows": a.repeats, "uncertainty": bool(a.uncertainty),
        "equal_sides": bool(a.equal_sides), "share_net": bool(a.share_net),
        "match": {"games_per_s": round(mgames, 2), "rounds_per_s": round(a.rounds / med_m, 1),
                  "us_per_round": round(1e6 * med_m / a.rounds, 2), "window_s": [round(x, 4) for x in msecs],
                  "nn_evals": mst["nn_evals"], "nn_batch_peak": mst["nn_batch_peak"],
                  "nn_precision": [kc.PRECISION_NAMES.get(p, "stand-in") for p in mst["nn_precision"]]},
        "selfplay": {"games_per_s": round(sgames, 2), "rounds_per_s": round(a.rounds / med_s, 1),
                     "us_per_round": round(1e6 * med_s / a.rounds, 2), "window_s": [round(x, 4) for x in ssecs],
                     "nn_evals": sst["nn_evals"]},
        "match_over_selfplay_round_time": round(med_m / med_s, 3),
    }))


if __name__ == "__main__":
    main()
