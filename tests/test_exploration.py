"""Variance-scaled exploration and noise pruning, the checks that need no GPU:
the two host entry points (csrc/explore.h, the sequences the search kernels run) against float64
restatements of the reference's lines, the parameter validation, and the config keys."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)

# The largest relative differences measured on the grids below between the f32 sequences and
# their float64 restatements (printed by the tests); each test asserts four times its figure.
# The factor's figure is set by the variance's subtraction (... / (pw + ws - 1) - u^2): at weight
# 600 with the second moment at the squared mean, a difference of 5e-4 is left of terms near 1,
# so the f32 roundings of those terms (6e-8) are 1e-4 of it.
MEASURED_FACTOR = 1.16e-5
MEASURED_PRUNE = 4.77e-7


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


def _f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------
# 1. The stdev factor.

def factor64(visits, ws, u, usq_avg, prior, prior_weight, scale):
    """getFpuValueForChildrenAssumeVisited searchexplorehelpers.cpp:256-277 in float64, on the
    f32 inputs."""
    ws, u, usq_avg, prior, prior_weight, scale = (_f32(v) for v in (ws, u, usq_avg, prior, prior_weight, scale))
    if visits <= 0 or ws <= 1:
        stdev = prior
    else:
        usq = u * u
        if usq_avg < usq:
            usq_avg = usq
        stdev = np.sqrt(max(0.0, ((usq + prior * prior) * prior_weight + usq_avg * ws) / (prior_weight + ws - 1.0)
                            - usq))
    return 1.0 + scale * (stdev / prior - 1.0)


PARAM_SETS = [(0.25, 1.0, 0.0), (0.40, 2.0, 0.85), (0.40, 2.0, 1.0)]


def test_stdev_factor_against_float64(L):
    worst = 0.0
    n = 0
    for prior, pw, scale in PARAM_SETS:
        over = dict(cpuct_utility_stdev_prior=prior, cpuct_utility_stdev_prior_weight=pw,
                    cpuct_utility_stdev_scale=scale)
        for ws in (0.5, 1.0, 1.0000001, 1.5, 2.0, 3.7, 10.0, 64.0, 150.25, 600.0):
            for u in np.linspace(-1.0, 1.0, 9):
                usq = _f32(u) * _f32(u)
                for usq_avg in [usq * (1.0 - 1e-6), usq] + list(usq + (1.0 - usq) * np.array([1e-6, 0.01, 0.3, 1.0])):
                    for visits in (0, 7):
                        got = kc.explore_stdev_factor(visits, ws, u, usq_avg, **over)
                        assert got.dtype == np.float32
                        if scale == 0.0:
                            assert got == np.float32(1.0) and np.float32(got).view(np.uint32) == 0x3F800000
                            continue
                        want = factor64(visits, ws, u, usq_avg, prior, pw, scale)
                        worst = max(worst, abs(float(got) - want) / abs(want))
                        n += 1
    print("stdev factor: largest relative difference to float64 %.3e over %d points" % (worst, n))
    assert n > 1000
    assert worst <= 4 * MEASURED_FACTOR


def test_stdev_factor_widens_where_the_utility_spreads(L):
    on = dict(cpuct_utility_stdev_scale=0.85)
    # a parent at or below weight 1, or without visits: the prior, factor 1
    assert kc.explore_stdev_factor(5, 1.0, 0.3, 0.9, **on) == np.float32(1.0)
    assert kc.explore_stdev_factor(0, 50.0, 0.3, 0.9, **on) == np.float32(1.0)
    # children that agree narrow the search, children that disagree widen it
    assert kc.explore_stdev_factor(100, 100.0, 0.2, 0.04, **on) < 1.0
    assert kc.explore_stdev_factor(100, 100.0, 0.0, 0.64, **on) > 1.0
    # a second-moment average below the squared mean counts as the squared mean
    a = kc.explore_stdev_factor(100, 100.0, 0.5, 0.2, **on)
    b = kc.explore_stdev_factor(100, 100.0, 0.5, 0.25, **on)
    assert a.view(np.uint32) == b.view(np.uint32)


# ---------------------------------------------------------------------------------------
# 2. Noise pruning.

def prune64(w, u, p, utility_scale=0.15, cap=float("inf")):
    """pruneNoiseWeight searchupdatehelpers.cpp:423-467 (with the caller's max(1e-30, prior),
    :191) in float64, on the f32 inputs."""
    w = [_f32(x) for x in w]
    u = [_f32(x) for x in u]
    p = [max(1e-30, _f32(x)) for x in p]
    utility_scale, cap = _f32(utility_scale), (cap if cap == float("inf") else _f32(cap))
    total = float(np.sum(w))
    if len(w) <= 1 or total <= 0.00001:
        return list(w), total
    usum = wsum = psum = 0.0
    out = []
    for old, ui, pi in zip(w, u, p):
        nw = old
        if wsum > 0 and psum > 0:
            gap = usum / wsum - ui
            if gap > 0:
                lenient = 2.0 * (wsum * pi / psum)
                if old > lenient:
                    sub = (old - lenient) * (1.0 - np.exp(-gap / utility_scale))
                    nw = old - min(sub, cap)
        usum += ui * nw
        wsum += nw
        psum += pi
        out.append(nw)
    return out, wsum


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if len(want) else 0.0


def _random_children(rng, n):
    # an expansion order: priors roughly descending, visits roughly following them, with
    # low-prior children that root noise over-visited
    p = np.sort(rng.dirichlet(np.full(n, 0.3)))[::-1].astype(np.float32) if n > 1 else np.ones(1, np.float32)
    w = (rng.gamma(1.0, 1.0, n) * (1.0 + 200.0 * p)).astype(np.float32) + np.float32(0.5)
    u = np.clip(rng.normal(0.0, 0.4, n), -1, 1).astype(np.float32)
    if n > 2:
        p[-1] = np.float32(1e-35)   # below the 1e-30 floor
        p[n // 2] = np.float32(-1.0)  # an illegal (masked) move's prior
        w[rng.integers(1, n)] *= np.float32(20.0)  # one over-visited child
    return w, u, p


HAND_MADE = {
    # descending priors, utilities rising along the order: no child lies below the average before it
    "nothing to prune": ([10, 5, 2, 1], [-0.2, -0.1, 0.0, 0.3], [0.5, 0.25, 0.15, 0.1], {}),
    "one over-visited bad child": ([40, 10, 30, 2], [0.3, 0.25, -0.6, 0.2], [0.6, 0.2, 0.01, 0.05], {}),
    "binding cap": ([40, 10, 30, 2], [0.3, 0.25, -0.6, 0.2], [0.6, 0.2, 0.01, 0.05], dict(noise_pruning_cap=1.5)),
    "tiny total": ([4e-6, 3e-6, 2e-6], [0.5, -0.5, -0.9], [0.9, 0.05, 0.05], {}),
}


def test_prune_noise_weight_against_float64(L):
    worst = 0.0
    pruned_sets = 0
    rng = np.random.default_rng(20240607)
    cases = [(name,) + c for name, c in HAND_MADE.items()]
    for n in (1, 2, 17, 65, 100):
        for rep in range(6):
            w, u, p = _random_children(rng, n)
            cases.append(("random n=%d #%d" % (n, rep), w, u, p, dict(noise_prune_utility_scale=[0.15, 0.05, 1.0][rep % 3])))
    for name, w, u, p, over in cases:
        got_w, got_t = kc.prune_noise_weight(w, u, p, use_noise_pruning=1, **over)
        want_w, want_t = prune64(w, u, p, utility_scale=over.get("noise_prune_utility_scale", 0.15),
                                 cap=over.get("noise_pruning_cap", float("inf")))
        w32 = np.asarray(w, np.float32)
        assert got_w.dtype == np.float32 and got_w.shape == w32.shape
        assert np.all(got_w <= w32) and np.all(got_w >= 0), name
        # a new weight is held to its old one: old - sub leaves little of a heavily pruned child, and
        # the roundings of old and sub are relative to them, not to what is left
        r = max(float(np.max(np.abs(got_w.astype(np.float64) - np.asarray(want_w)) / w32)) if len(w32) else 0.0,
                _rel([got_t], [want_t]))
        worst = max(worst, r)
        changed = int(np.sum(got_w != w32))
        pruned_sets += changed > 0
        if name == "nothing to prune" or name == "tiny total" or len(w32) <= 1:
            assert changed == 0 and got_w.tobytes() == w32.tobytes(), name  # the input bits
        if name == "one over-visited bad child":
            assert changed == 1 and got_w[2] < 0.2 * w32[2], (name, got_w)
        if name == "binding cap":
            assert changed == 1 and got_w[2] == np.float32(30 - 1.5), (name, got_w)
        assert r <= 4 * MEASURED_PRUNE, (name, r)
    print("noise pruning: largest relative difference to float64 %.3e over %d child sets (%d pruned)" %
          (worst, len(cases), pruned_sets))
    assert pruned_sets >= 20


def test_prune_noise_weight_exact_cases(L):
    # n <= 1 and totals <= 1e-5 come back bit for bit, with their in-order f32 sum
    for w in ([], [3.25], [4e-6, 3e-6, 2e-6], [1e-5, 0.0]):
        w32 = np.asarray(w, np.float32)
        got_w, got_t = kc.prune_noise_weight(w32, np.linspace(0.9, -0.9, len(w32)), np.full(len(w32), 0.01), use_noise_pruning=1)
        assert got_w.tobytes() == w32.tobytes()
        tot = np.float32(0.0)
        for x in w32:
            tot = np.float32(tot + x)
        assert got_t.view(np.uint32) == tot.view(np.uint32)
    # the first child is never pruned, and the total is the scan's own running sum
    got_w, got_t = kc.prune_noise_weight([7, 100, 3], [0.9, -0.9, 0.1], [0.9, 1e-6, 0.05], use_noise_pruning=1)
    assert got_w[0] == np.float32(7) and got_w[1] < 1.0
    tot = np.float32(0.0)
    for x in got_w:
        tot = np.float32(tot + x)
    assert got_t.view(np.uint32) == tot.view(np.uint32)


# ---------------------------------------------------------------------------------------
# 3. Validation: the parameter block and the config keys.

def test_defaults_are_off_with_the_reference_values(L):
    d = kc.default_exploration_params()
    assert d.use_noise_pruning == 0 and d.cpuct_utility_stdev_scale == 0.0
    assert d.cpuct_utility_stdev_prior == np.float32(0.40) and d.cpuct_utility_stdev_prior_weight == 2.0
    assert d.noise_prune_utility_scale == np.float32(0.15) and d.noise_pruning_cap == np.float32(FLT_MAX)
    assert ctypes.sizeof(kc.ExplorationParams) == 24


BAD_PARAMS = [
    ("use_noise_pruning", 2), ("use_noise_pruning", -1),
    ("noise_prune_utility_scale", 0.0005), ("noise_prune_utility_scale", 10.5), ("noise_prune_utility_scale", float("nan")),
    ("noise_pruning_cap", -1.0), ("noise_pruning_cap", float("inf")), ("noise_pruning_cap", float("nan")),
    ("cpuct_utility_stdev_prior", -0.1), ("cpuct_utility_stdev_prior", 10.5), ("cpuct_utility_stdev_prior", float("nan")),
    ("cpuct_utility_stdev_prior_weight", -1.0), ("cpuct_utility_stdev_prior_weight", 101.0),
    ("cpuct_utility_stdev_prior_weight", float("inf")),
    ("cpuct_utility_stdev_scale", -0.1), ("cpuct_utility_stdev_scale", 1.5), ("cpuct_utility_stdev_scale", float("nan")),
]


@pytest.mark.parametrize("name,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_out_of_range_parameters_are_refused_by_name(L, name, value):
    with pytest.raises(kc.CoffeeError, match=name):
        kc.explore_stdev_factor(5, 3.0, 0.1, 0.2, **{name: value})
    with pytest.raises(kc.CoffeeError, match=name):
        kc.prune_noise_weight([1, 2], [0, 0], [0.5, 0.5], **{name: value})


def test_prior_zero_needs_scale_zero_and_null_handles_are_refused(L):
    with pytest.raises(kc.CoffeeError, match="cpuct_utility_stdev_prior"):
        kc.explore_stdev_factor(5, 3.0, 0.1, 0.2, cpuct_utility_stdev_prior=0.0, cpuct_utility_stdev_scale=0.5)
    assert kc.explore_stdev_factor(5, 3.0, 0.1, 0.2, cpuct_utility_stdev_prior=0.0) == np.float32(1.0)
    p = kc.default_exploration_params()
    assert L.coffee_selfplay_set_exploration(None, ctypes.byref(p)) == -1
    assert L.coffee_analysis_set_exploration(None, ctypes.byref(p)) == -1
    for side in (-1, 0, 1, 2):
        assert L.coffee_match_set_exploration(None, side, ctypes.byref(p)) == -1
    n = ctypes.c_int()
    assert L.coffee_selfplay_game_tree_priors(None, 0, 4, None, None, None, ctypes.byref(n)) == -1


@pytest.fixture(scope="module")
def dump(L, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("explcfg") / "exploration_config_dump")
    libdir = os.path.dirname(kc.LIB_PATH)  # linked as the katago program is (csrc/Makefile)
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe,
                    os.path.join(REPO, "tests", "helpers", "exploration_config_dump.cpp"),
                    "-L" + libdir, "-lkatacoffee", "-Wl,-rpath," + libdir], check=True)

    def run(text, tmp_path):
        cfg = tmp_path / "c.cfg"
        cfg.write_text(text)
        r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, timeout=30)
        # (%.9g round-trips an f32: back to the f32 it printed)
        return r.returncode, [[float(np.float32(x)) for x in ln.split()] for ln in r.stdout.splitlines()], r.stderr
    return run


def test_config_keys_and_per_bot_precedence(dump, tmp_path):
    rc, rows, err = dump("maxVisits = 50\n", tmp_path)
    assert rc == 0, err
    d = kc.default_exploration_params()
    want = [0.0, d.noise_prune_utility_scale, d.noise_pruning_cap, d.cpuct_utility_stdev_prior,
            d.cpuct_utility_stdev_prior_weight, 0.0]
    assert rows == [want] * 3
    rc, rows, err = dump("cpuctUtilityStdevPrior = 0.4\ncpuctUtilityStdevPriorWeight = 2.0\ncpuctUtilityStdevScale = 0.85\n"
                         "useNoisePruning = true\nnoisePruneUtilityScale = 0.15\nnoisePruningCap = 1e50\n"
                         "cpuctUtilityStdevScale1 = 0.5\nuseNoisePruning1 = false\nnoisePruningCap0 = 3.5\n"
                         "noisePruneUtilityScale1 = 0.3\ncpuctUtilityStdevPrior0 = 0.25\ncpuctUtilityStdevPriorWeight1 = 7\n",
                         tmp_path)
    assert rc == 0, err
    plain, b0, b1 = rows
    f = lambda x: float(np.float32(x))
    assert plain == [1.0, f(0.15), FLT_MAX, f(0.4), 2.0, f(0.85)]  # a cap above FLT_MAX is FLT_MAX
    assert b0 == [1.0, f(0.15), 3.5, 0.25, 2.0, f(0.85)]
    assert b1 == [0.0, f(0.3), FLT_MAX, f(0.4), 7.0, 0.5]


BAD_KEYS = [("cpuctUtilityStdevPrior", "-1"), ("cpuctUtilityStdevPrior", "11"), ("cpuctUtilityStdevPriorWeight", "-0.5"),
            ("cpuctUtilityStdevPriorWeight", "101"), ("cpuctUtilityStdevScale", "-0.1"), ("cpuctUtilityStdevScale", "1.01"),
            ("noisePruneUtilityScale", "0.0001"), ("noisePruneUtilityScale", "11"), ("noisePruningCap", "-2"),
            ("noisePruningCap", "lots"), ("cpuctUtilityStdevScale", "nan")]


@pytest.mark.parametrize("suffix", ["", "0", "1"])
@pytest.mark.parametrize("key,value", BAD_KEYS, ids=["%s=%s" % b for b in BAD_KEYS])
def test_out_of_range_config_keys_are_refused_by_key(dump, tmp_path, key, value, suffix):
    rc, _, err = dump("%s%s = %s\n" % (key, suffix, value), tmp_path)
    assert rc == 1 and key + suffix in err, (rc, err)


def test_config_prior_zero_with_scale_is_refused(dump, tmp_path):
    rc, _, err = dump("cpuctUtilityStdevPrior = 0\ncpuctUtilityStdevScale = 0.5\n", tmp_path)
    assert rc == 1 and "cpuctUtilityStdevPrior" in err, (rc, err)
    rc, _, err = dump("cpuctUtilityStdevPrior = 0\n", tmp_path)
    assert rc == 0, err
