"""Wide root noise and futile-visit pruning, the checks that need no GPU: the two
host entry points (csrc/rootsearch.h, the sequences the search kernels run) against float64
restatements of the reference's lines, the statistics and the coordinates of the noise draws, the
parameter validation, and the config keys of all four commands."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest relative difference measured on the grid below between the f32 smoothed prior
# (dpow: dexp(y * dlog(x))) and prior ** (1 / (4 w + 1)) in float64 (printed by the test, which
# asserts four times the figure).  The figure is the rounding of the f32 product y * log(x), up
# to 13.8 at prior 1e-6, ahead of the exponential: 13.8 * 6e-8 = 8e-7.
MEASURED_SMOOTHED = 8.61e-7

SEED, SLOT, GAME, TURN = 0x5EED, 3, 2, 9


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


def _f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------
# 1. Wide root noise.

def test_smoothed_prior_against_float64(L):
    """Largest relative difference measured: 8.61e-7 (MEASURED_SMOOTHED); asserted: four times it."""
    worst, n = 0.0, 0
    priors = np.concatenate([np.logspace(-6, 0, 61), [0.3, 0.5, 0.999, 1.0]])
    for w in (0.04, 0.5, 5.0):
        for p in priors:
            got, _ = kc.wide_root_noise(SEED, SLOT, GAME, TURN, 5, 7, p, wide_root_noise=w)
            assert got.dtype == np.float32
            want = _f32(p) ** (1.0 / (4.0 * _f32(w) + 1.0))
            worst = max(worst, abs(float(got) - want) / want)
            n += 1
    print("smoothed prior: largest relative difference to float64 %.3e over %d points" % (worst, n))
    assert n >= 180
    assert worst <= 4 * MEASURED_SMOOTHED
    # an illegal move's prior is never smoothed by the kernels; 0 stays 0, and off is the identity
    assert kc.wide_root_noise(SEED, SLOT, GAME, TURN, 5, 7, 0.0, wide_root_noise=0.5)[0] == 0.0
    got = kc.wide_root_noise(SEED, SLOT, GAME, TURN, 5, 7, 0.123)
    assert got == (np.float32(0.123), np.float32(0.0))


def test_bonus_is_a_fair_coin_times_a_half_normal(L):
    w = 0.5
    b = np.array([[float(kc.wide_root_noise(SEED, SLOT, GAME, TURN, rv, pos, 0.1, wide_root_noise=w)[1])
                   for pos in range(64)] for rv in range(1, 65)])
    assert b.shape == (64, 64) and np.all(b >= 0.0)
    share = float((b > 0).mean())
    mean = float((b[b > 0] / _f32(w)).mean())
    print("bonus: share with a bonus %.4f, mean |gauss| %.4f" % (share, mean))
    assert 0.45 <= share <= 0.55
    assert abs(mean - 0.798) <= 0.05
    # the bonus scales with the setting: the draws are the same ones
    b2 = np.array([float(kc.wide_root_noise(SEED, SLOT, GAME, TURN, 1, pos, 0.1, wide_root_noise=0.25)[1])
                   for pos in range(64)])
    np.testing.assert_allclose(b2, b[0] * 0.5, rtol=1e-6, atol=0.0)


def test_noise_depends_on_its_coordinates_alone(L):
    def bonuses(seed=SEED, slot=SLOT, game=GAME, turn=TURN, rv=17, prior=0.1, first=0):
        return [float(kc.wide_root_noise(seed, slot, game, turn, rv, pos, prior, wide_root_noise=0.5)[1])
                for pos in range(first, first + 32)]
    base = bonuses()
    assert sum(x > 0 for x in base) >= 8
    assert bonuses() == base
    assert bonuses(prior=0.9) == base and bonuses(prior=1e-5) == base
    for other in (dict(turn=TURN + 1), dict(rv=18), dict(first=1), dict(seed=SEED + 1), dict(slot=SLOT + 1),
                  dict(game=GAME + 1)):
        assert bonuses(**other) != base, other
    # (a shifted window holds the same draws one position on: the position is a coordinate)
    assert bonuses(first=1)[:-1] == base[1:]


# ---------------------------------------------------------------------------------------
# 2. Futile visits.

def futile64(thr, max_w, ws, pvis, left, ev, cv, w, is_new):
    """getExploreSelectionValueOfChild searchexplorehelpers.cpp:140-147 and
    getNewExploreSelectionValue :194-201 in float64 on the f32 inputs: (lhs, need)."""
    thr, max_w, ws, w = (_f32(v) for v in (thr, max_w, ws, w))
    wpv = ws / pvis
    required = thr * max_w
    if is_new:
        return float(left), required * (1.0 / wpv)
    return float(cv + left), required * ((ev + 1.0) / (w + wpv))


FUTILE_GRID = list(itertools.product(
    (0.01, 0.15, 0.4, 1.0),                    # threshold
    (0.73, 7.31, 41.7, 233.3),                 # largest child weight
    ((12.9, 13), (57.3, 50), (310.7, 333)),    # the root's weight sum and visits
    (0, 1, 3, 14, 97, 400),                    # visits left
    ((0, 0, 0.0), (1, 1, 0.91), (3, 5, 4.37), (20, 20, 26.3), (77, 90, 61.9)),  # edge visits, child visits, weight
))


def test_futile_visits_against_float64(L):
    skipped = checked = futile = 0
    for thr, max_w, (ws, pvis), left, (ev, cv, w) in FUTILE_GRID:
        for is_new in (False, True):
            if is_new and (ev, cv) != (0, 0):
                continue
            lhs, need = futile64(thr, max_w, ws, pvis, left, ev, cv, w, is_new)
            if abs(lhs - need) < 1e-5 * max(abs(lhs), abs(need)):
                skipped += 1
                continue
            got = kc.futile_visits(max_w, ws, pvis, left, ev, cv, w, is_new, futile_visits_threshold=thr)
            assert got == (lhs < need), (thr, max_w, ws, pvis, left, ev, cv, w, is_new, lhs, need)
            checked += 1
            futile += got
            assert not kc.futile_visits(max_w, ws, pvis, left, ev, cv, w, is_new)  # off: never
    total = skipped + checked
    print("futile visits: %d points, %d futile, %d skipped as too close to call" % (total, futile, skipped))
    assert total >= 1500 and skipped <= 0.02 * total
    assert 0.1 * checked <= futile <= 0.9 * checked


# ---------------------------------------------------------------------------------------
# 3. Parameters.

def test_defaults_are_off(L):
    p = kc.default_root_search_params()
    assert (p.wide_root_noise, p.futile_visits_threshold) == (0.0, 0.0)
    assert ctypes.sizeof(kc.RootSearchParams) == 8


BAD_PARAMS = [("wide_root_noise", -0.01), ("wide_root_noise", 5.5), ("wide_root_noise", float("nan")),
              ("wide_root_noise", float("inf")), ("futile_visits_threshold", 0.005), ("futile_visits_threshold", -0.1),
              ("futile_visits_threshold", 1.01), ("futile_visits_threshold", float("nan"))]


@pytest.mark.parametrize("name,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_out_of_range_parameters_are_refused_by_name(L, name, value):
    with pytest.raises(kc.CoffeeError, match=name):
        kc.wide_root_noise(1, 0, 0, 0, 1, 0, 0.5, **{name: value})
    with pytest.raises(kc.CoffeeError, match=name):
        kc.futile_visits(1.0, 2.0, 2, 1, **{name: value})


def test_edges_of_the_ranges_and_null_handles(L):
    for over in (dict(wide_root_noise=5.0), dict(futile_visits_threshold=0.01), dict(futile_visits_threshold=1.0)):
        kc.futile_visits(1.0, 2.0, 2, 1, **over)
    with pytest.raises(kc.CoffeeError, match="pos"):
        kc.wide_root_noise(1, 0, 0, 0, 1, -1, 0.5, wide_root_noise=0.5)
    p = kc.default_root_search_params(wide_root_noise=0.04)
    assert L.coffee_selfplay_set_root_search(None, ctypes.byref(p)) == -1
    assert L.coffee_analysis_set_root_search(None, ctypes.byref(p)) == -1
    for side in (-1, 0, 1, 2):
        assert L.coffee_match_set_root_search(None, side, ctypes.byref(p)) == -1
    out = ctypes.c_int()
    assert L.coffee_futile_visits(None, 1.0, 1.0, 1, 1, 0, 0, 0.0, 0, ctypes.byref(out)) == -1
    assert L.coffee_futile_visits(ctypes.byref(p), 1.0, 1.0, 1, 1, 0, 0, 0.0, 0, None) == -1


# ---------------------------------------------------------------------------------------
# 4. Config keys.

@pytest.fixture(scope="module")
def dump(L, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rscfg") / "root_search_config_dump")
    libdir = os.path.dirname(kc.LIB_PATH)  # linked as the katago program is (csrc/Makefile)
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe,
                    os.path.join(REPO, "tests", "helpers", "root_search_config_dump.cpp"),
                    "-L" + libdir, "-lkatacoffee", "-Wl,-rpath," + libdir], check=True)

    def run(text, tmp_path):
        cfg = tmp_path / "c.cfg"
        cfg.write_text(text)
        r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, timeout=30)
        return r.returncode, [[float(np.float32(x)) for x in ln.split()] for ln in r.stdout.splitlines()], r.stderr
    return run


def test_config_keys_and_per_bot_precedence(dump, tmp_path):
    rc, rows, err = dump("maxVisits = 50\n", tmp_path)
    assert rc == 0, err
    assert rows == [[0.0, 0.0]] * 3  # absent keys: off, for analysis too
    rc, rows, err = dump("wideRootNoise = 0.04\nfutileVisitsThreshold = 0.15\n", tmp_path)
    assert rc == 0, err
    assert rows == [[_f32(0.04), _f32(0.15)]] * 3
    rc, rows, err = dump("wideRootNoise = 0.04\nwideRootNoise1 = 0.5\nfutileVisitsThreshold0 = 0.25\n", tmp_path)
    assert rc == 0, err
    assert rows == [[_f32(0.04), 0.0], [_f32(0.04), 0.25], [0.5, 0.0]]
    for cfg in ("analysis_coffee5.cfg", "match_coffee5.cfg"):  # the shipped configs keep both off
        rc, rows, err = dump(open(os.path.join(REPO, "configs", cfg)).read(), tmp_path)
        assert rc == 0 and rows == [[0.0, 0.0]] * 3, (cfg, err)
        assert "# wideRootNoise" in open(os.path.join(REPO, "configs", cfg)).read()


BAD_KEYS = [("wideRootNoise", "-0.1"), ("wideRootNoise", "5.01"), ("wideRootNoise", "nan"), ("wideRootNoise", "wide"),
            ("futileVisitsThreshold", "0"), ("futileVisitsThreshold", "0.009"), ("futileVisitsThreshold", "1.5"),
            ("futileVisitsThreshold", "0.2x")]


@pytest.mark.parametrize("suffix", ["", "0", "1"])
@pytest.mark.parametrize("key,value", BAD_KEYS, ids=["%s=%s" % b for b in BAD_KEYS])
def test_out_of_range_config_keys_are_refused_by_key(dump, tmp_path, key, value, suffix):
    rc, _, err = dump("%s%s = %s\n" % (key, suffix, value), tmp_path)
    assert rc == 1 and key + suffix in err, (rc, err)
