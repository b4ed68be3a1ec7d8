"""Per-side match settings (coffee_match_create2, kc.Match(sides=...), coffee_match_elo and the
config layer of `katago match`), the checks that need no GPU: every rejection precedes the
first device call."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


def _options(base, per_side=1, share_net=0, side0=None, side1=None, unc0=None, unc1=None):
    o = kc.MatchOptions()
    o.per_side, o.share_net = per_side, share_net
    for i, (over, unc) in enumerate(((side0, unc0), (side1, unc1))):
        o.side[i].search = kc.SearchParams.from_buffer_copy(base)
        o.side[i].unc = kc.default_uncertainty_params()
        for k, v in (over or {}).items():
            setattr(o.side[i].search, k, v)
        for k, v in (unc or {}).items():
            setattr(o.side[i].unc, k, v)
    return o


def _create2(L, node_cap=128, paths=(None, None), opts=True, **okw):
    cfg = kc.MatchConfig()
    cfg.x, cfg.y, cfg.win_len = 5, 5, 4
    cfg.num_games = 4
    cfg.node_cap = node_cap
    cfg.seed = 1
    cfg.search = kc.default_match_params(max_visits=8)
    keep = [p.encode() if p else None for p in paths]
    cfg.model_path[0], cfg.model_path[1] = keep
    o = _options(cfg.search, **okw) if opts else None
    h = ctypes.c_void_p()
    rc = L.coffee_match_create2(ctypes.byref(cfg), ctypes.byref(o) if o is not None else None, ctypes.byref(h))
    msg = L.coffee_last_error().decode()
    if rc == 0:  # a GPU is present and nothing was wrong
        L.coffee_match_destroy(h)
    return rc, msg


# the settings validateMatchConfig rejects, on one side only
FORBIDDEN = [("cheap_search_prob", 0.25), ("reduce_visits", 1), ("early_fork_game_prob", 0.04),
             ("fork_game_prob", 0.01), ("side_position_prob", 0.02), ("record_tree_positions", 1),
             ("policy_surprise_data_weight", 0.5), ("value_surprise_data_weight", 0.1)]


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name,value", FORBIDDEN, ids=[n for n, _ in FORBIDDEN])
def test_a_sides_forbidden_setting_is_rejected_by_side_and_name(L, side, name, value):
    rc, msg = _create2(L, **{"side%d" % side: {name: value}})
    assert rc == -1, (rc, msg)  # COFFEE_EINVAL
    assert "side %d" % side in msg and name in msg, msg


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("over,word", [({"max_visits": 0}, "max_visits"),
                                       ({"root_num_symmetries_to_sample": 5}, "root_num_symmetries_to_sample"),
                                       ({"root_num_symmetries_to_sample": 0}, "root_num_symmetries_to_sample")])
def test_a_sides_out_of_range_search_value_is_rejected(L, side, over, word):
    rc, msg = _create2(L, **{"side%d" % side: over})
    assert rc == -1 and "side %d" % side in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("unc,word", [({"use_uncertainty": 2}, "use_uncertainty"),
                                      ({"uncertainty_coeff": 0.0}, "uncertainty_coeff"),
                                      ({"uncertainty_coeff": float("nan")}, "uncertainty_coeff"),
                                      ({"uncertainty_exponent": 2.5}, "uncertainty_exponent"),
                                      ({"uncertainty_max_weight": 0.5}, "uncertainty_max_weight")])
def test_a_sides_uncertainty_out_of_range_is_rejected(L, side, unc, word):
    rc, msg = _create2(L, **{"unc%d" % side: unc})
    assert rc == -1 and "side %d" % side in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name,value", [("init_games_with_policy", 1), ("policy_init_area_prop", 0.5),
                                        ("policy_init_area_temperature", 2.0)])
def test_a_game_level_field_must_equal_the_configs(L, side, name, value):
    rc, msg = _create2(L, **{"side%d" % side: {name: value}})
    assert rc == -1 and "side %d" % side in msg and name in msg, (rc, msg)


def test_share_net_needs_equal_model_paths(L):
    for paths in (("a.cfnn", "b.cfnn"), (None, "b.cfnn"), ("a.cfnn", None)):
        rc, msg = _create2(L, paths=paths, share_net=1)
        assert rc == -1 and "share_net" in msg and "model_path" in msg, (paths, rc, msg)
    # also without per-side settings
    rc, msg = _create2(L, paths=("a.cfnn", "b.cfnn"), share_net=1, per_side=0)
    assert rc == -1 and "share_net" in msg, (rc, msg)
    # both NULL counts as equal: the next failure is a HIP one (no device), or none
    rc, msg = _create2(L, share_net=1)
    assert rc in (0, -2), (rc, msg)


def test_a_sides_max_visits_must_fit_the_node_pool(L):
    # node_cap 128: max_visits + 4 <= 128, the rule coffee_match_create applies to cfg->search
    rc, msg = _create2(L, side1={"max_visits": 125})
    assert rc == -1 and "side 1" in msg and "max_visits" in msg and "node_cap" in msg, (rc, msg)
    rc, msg = _create2(L, side0={"max_visits": 125})
    assert rc == -1 and "side 0" in msg and "max_visits" in msg, (rc, msg)
    rc, msg = _create2(L, side0={"max_visits": 124}, side1={"max_visits": 124})
    assert rc in (0, -2), (rc, msg)
    # node_cap 0: the default comes from the larger side, so any pair passes this check
    rc, msg = _create2(L, node_cap=0, side0={"max_visits": 4}, side1={"max_visits": 5000})
    assert rc in (0, -2), (rc, msg)


def test_flags_must_be_0_or_1_and_null_options_are_todays_create(L):
    rc, msg = _create2(L, per_side=2)
    assert rc == -1 and "per_side" in msg, (rc, msg)
    rc, msg = _create2(L, opts=False)
    assert rc in (0, -2), (rc, msg)
    # per_side 0 ignores the sides, whatever they hold
    rc, msg = _create2(L, per_side=0, side0={"cheap_search_prob": 0.5})
    assert rc in (0, -2), (rc, msg)


def test_abi_version_and_struct_sizes(L):
    assert L.coffee_abi_version() == 108
    assert ctypes.sizeof(kc.SearchParams) == 212
    assert ctypes.sizeof(kc.MatchSide) == 228
    assert ctypes.sizeof(kc.MatchOptions) == 464
    # and the C compiler's view of the header agrees
    src = ('#include "%s"\n#include <stdio.h>\nint main(void){printf("%%zu %%zu\\n",sizeof(coffee_match_side),'
           'sizeof(coffee_match_options));return 0;}\n' % os.path.join(REPO, "include", "katacoffee.h"))
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["228", "464"]


# ---- kc.Match(sides=...) error paths ----

def test_python_sides_error_paths(L):
    with pytest.raises(kc.CoffeeError, match="pair"):
        kc.Match(5, 5, 4, num_games=2, sides=({},))
    with pytest.raises(kc.CoffeeError, match="no_such_field"):
        kc.Match(5, 5, 4, num_games=2, sides=({"no_such_field": 1}, {}))
    with pytest.raises(kc.CoffeeError, match=r"sides\[1\]"):
        kc.Match(5, 5, 4, num_games=2, sides=({}, 7))
    with pytest.raises(kc.CoffeeError, match="SearchParams"):
        kc.Match(5, 5, 4, num_games=2, sides=({}, ({"max_visits": 3}, None)))
    # the library's own rejections arrive as CoffeeError naming side and field
    with pytest.raises(kc.CoffeeError, match=r"side 1.*cheap_search_prob"):
        kc.Match(5, 5, 4, num_games=2, max_visits=8, node_cap=128, sides=({}, {"cheap_search_prob": 0.5}))
    with pytest.raises(kc.CoffeeError, match=r"side 0.*uncertainty_coeff"):
        kc.Match(5, 5, 4, num_games=2, max_visits=8, node_cap=128,
                 sides=((None, kc.default_uncertainty_params(uncertainty_coeff=2.0)), {}))
    with pytest.raises(kc.CoffeeError, match="share_net"):
        kc.Match(5, 5, 4, num_games=2, max_visits=8, baseline_path="a.cfnn", candidate_path="b.cfnn", share_net=True)


# ---- coffee_match_elo ----

def _elo_numpy(W, D, Lo):
    W, D, Lo = np.float64(W), np.float64(D), np.float64(Lo)
    N = W + D + Lo
    p = (W + D / 2) / N
    var = (W * (1 - p) ** 2 + D * (0.5 - p) ** 2 + Lo * p ** 2) / N
    se = np.sqrt(var / N)

    def elo(x):
        if x <= 0:
            return -np.inf
        if x >= 1:
            return np.inf
        return -400.0 * np.log10(1.0 / x - 1.0)
    los = 0.5 * math.erfc(-(W - Lo) / math.sqrt(2 * (W + Lo))) if W + Lo > 0 else 0.5
    return {"score": p, "elo": elo(p), "elo_lo": elo(p - 1.96 * se), "elo_hi": elo(p + 1.96 * se), "los": los}


@pytest.mark.parametrize("wdl", [(10, 0, 0), (0, 0, 10), (0, 7, 0), (37, 11, 52)])
def test_match_elo_against_the_formulas(L, wdl):
    got, want = kc.match_elo(*wdl), _elo_numpy(*wdl)
    for k, w in want.items():
        g = got[k]
        if np.isinf(w):
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= 1e-9, (k, g, w)
    if wdl == (37, 11, 52):  # a finite case really is one
        assert all(np.isfinite(v) for v in got.values()) and got["elo_lo"] < got["elo"] < got["elo_hi"]
    if wdl == (10, 0, 0):
        assert got["elo"] == np.inf and got["elo_hi"] == np.inf
    if wdl == (0, 0, 10):
        assert got["elo"] == -np.inf and got["elo_lo"] == -np.inf
    if wdl == (0, 7, 0):
        assert got["score"] == 0.5 and got["los"] == 0.5 and got["elo"] == 0.0


def test_match_elo_refuses_no_games(L):
    with pytest.raises(kc.CoffeeError, match="no games"):
        kc.match_elo(0, 0, 0)
    with pytest.raises(kc.CoffeeError):
        kc.match_elo(-1, 2, 0)
    # outputs are optional
    assert L.coffee_match_elo(1, 0, 0, None, None, None, None, None) == 0


# ---- the config layer of `katago match`: key<i> over key over the default ----

@pytest.fixture(scope="module")
def dump(L, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("matchcfg") / "match_config_dump")
    libdir = os.path.dirname(kc.LIB_PATH)  # linked as the katago program is (csrc/Makefile)
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe, os.path.join(REPO, "tests", "helpers", "match_config_dump.cpp"),
                    "-L" + libdir, "-lkatacoffee", "-Wl,-rpath," + libdir], check=True)

    def run(text, tmp_path):
        cfg = tmp_path / "c.cfg"
        cfg.write_text(text)
        r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, timeout=30)
        return r.returncode, [ln.split() for ln in r.stdout.splitlines()], r.stderr
    return run


def test_suffix_precedence(dump, tmp_path):
    rc, bots, err = dump("numBots = 2\nbotName0 = base\nbotName1 = wide\nnnModelFile = net.cfnn\n"
                         "cpuctExploration = 0.9\ncpuctExploration1 = 1.3\nmaxVisits1 = 300\n"
                         "useUncertainty1 = true\nuncertaintyCoeff = 0.5\nuncertaintyCoeff1 = 0.125\n", tmp_path)
    assert rc == 0, err
    b0, b1 = bots
    # bot 1: the suffixed key beats the plain one
    assert b1[0] == "wide" and b1[1] == "net.cfnn" and int(b1[2]) == 300 and float(b1[3]) == pytest.approx(1.3)
    assert int(b1[5]) == 1 and float(b1[6]) == 0.125
    # bot 0 falls back to the unsuffixed key, then to the default (150 visits, uncertainty off)
    assert b0[0] == "base" and b0[1] == "net.cfnn" and int(b0[2]) == 150 and float(b0[3]) == pytest.approx(0.9)
    assert int(b0[5]) == 0 and float(b0[6]) == 0.5
    d = kc.default_uncertainty_params()
    assert float(b0[7]) == d.uncertainty_exponent and float(b0[8]) == d.uncertainty_max_weight


def test_defaults_and_per_bot_models(dump, tmp_path):
    rc, bots, err = dump("nnModelFile0 = a.cfnn\nnnModelFile1 = b.cfnn\n", tmp_path)
    assert rc == 0, err
    p = kc.default_match_params()
    for i, b in enumerate(bots):
        assert b[0] == "bot%d" % i and b[1] == ("a.cfnn", "b.cfnn")[i]
        assert int(b[2]) == p.max_visits and float(b[3]) == pytest.approx(p.cpuct_exploration) and int(b[4]) == 0


@pytest.mark.parametrize("n", ["3", "1"])
def test_num_bots_other_than_two_is_refused(dump, tmp_path, n):
    rc, _, err = dump("numBots = %s\n" % n, tmp_path)
    assert rc == 1 and "numBots" in err and "2" in err, (rc, err)


def test_bad_suffixed_value_names_the_suffixed_key(dump, tmp_path):
    rc, _, err = dump("maxVisits1 = many\n", tmp_path)
    assert rc == 1 and "maxVisits1" in err, (rc, err)
    rc, _, err = dump("uncertaintyCoeff0 = 7\n", tmp_path)
    assert rc == 1 and "uncertaintyCoeff0" in err, (rc, err)


# ---- the command line's usage errors (no device is touched) ----

def test_usage_errors(L):
    exe = os.path.join(REPO, "katacoffee_amd", "katago")
    r = subprocess.run([exe, "nosuchcommand"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: katago selfplay" in r.stderr
    r = subprocess.run([exe, "match"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: katago match -config" in r.stderr
    r = subprocess.run([exe, "match", "-config", "/nonexistent.cfg", "-sgf-output-dir", "/tmp/x"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read config" in r.stderr
