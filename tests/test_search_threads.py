"""Parallel playouts per search, host side: the virtual-loss valuation of vloss.h
run through coffee_virtual_loss against a float64 restatement, and the config keys of
`katago analysis`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vl64(per_thread, vl, mover, u, w):
    """getExploreSelectionValueOfChild searchexplorehelpers.cpp:125-134 in float64 (utility radius 1)."""
    vlw = float(vl) * float(per_thread)
    loss = -1.0 if mover == 2 else 1.0
    frac = vlw / (vlw + max(0.25, float(w)))
    return float(u) + (loss - float(u)) * frac, float(w) + vlw


WEIGHTS = [0.0, 0.1, 0.25, 0.2500001, 0.5, 1.0, 3.7, 17.0, 64.5, 199.0, 600.0]
UTILITIES = [-1.0, -0.73, -0.25, -1e-3, 0.0, 1e-3, 0.31, 0.999, 1.0]


def test_virtual_loss_against_float64():
    """vl in {1, 2, 5, 32}, per-thread in {1, 3}, weights 0 .. 600 with 0 and 0.25, utilities -1 .. 1,
    both movers.  The utility is compared relative to the span of utilities it interpolates in
    (|u| + 1 >= 1: the result itself may cancel to 0), the weight relative to itself.  Largest
    difference measured on the CPU: 1.380e-07 (utility), 5.073e-08 (weight) -- a handful of f32
    roundings of 2^-24 each; asserted at four times the larger, 5.52e-07."""
    worst_u = worst_w = 0.0
    for vl in (1, 2, 5, 32):
        for per in (1.0, 3.0):
            for mover in (1, 2):
                for w in WEIGHTS:
                    for u in UTILITIES:
                        gu, gw = kc.virtual_loss(per, vl, mover, u, w)
                        wu, ww = _vl64(per, vl, mover, np.float32(u), np.float32(w))
                        worst_u = max(worst_u, abs(float(gu) - wu) / (abs(wu) + 1.0))
                        worst_w = max(worst_w, abs(float(gw) - ww) / ww)
                        # towards the mover's loss, never past it
                        assert (-1.0 <= gu <= np.float32(u)) if mover == 2 else (np.float32(u) <= gu <= 1.0)
    print("virtual loss vs float64: largest relative difference %.3e (utility), %.3e (weight)" % (worst_u, worst_w))
    assert max(worst_u, worst_w) <= 5.52e-07


def test_no_virtual_loss_returns_the_inputs_bit_for_bit():
    for mover in (1, 2):
        for w in WEIGHTS + [np.float32(1e-30), np.float32(3e38)]:
            for u in UTILITIES + [-0.0]:
                gu, gw = kc.virtual_loss(3.0, 0, mover, u, w)
                assert gu.tobytes() == np.float32(u).tobytes() and gw.tobytes() == np.float32(w).tobytes()


def test_virtual_loss_rejects_bad_arguments():
    L = kc.lib()
    u, w = ctypes.c_float(), ctypes.c_float()
    f = ctypes.c_float
    assert L.coffee_virtual_loss(f(1.0), 1, 0, f(0.0), f(1.0), ctypes.byref(u), ctypes.byref(w)) == -1
    assert L.coffee_virtual_loss(f(0.0), 1, 1, f(0.0), f(1.0), ctypes.byref(u), ctypes.byref(w)) == -1
    assert L.coffee_virtual_loss(f(float("nan")), 1, 1, f(0.0), f(1.0), ctypes.byref(u), ctypes.byref(w)) == -1
    assert L.coffee_virtual_loss(f(1.0), 1, 2, f(0.5), f(1.0), None, None) == 0
    assert L.coffee_analysis_set_search_threads(None, 4, f(1.0)) == -1
    assert L.coffee_analysis_search_threads_info(None, None) == -1
    assert L.coffee_analysis_round_paths(None, 0, None) == -1
    assert ctypes.sizeof(kc.RoundPaths) == 8 + 32 * (8 + 2 * 4 * 102) and ctypes.sizeof(kc.SearchThreadsInfo) == 32


# ---------------------------------------------------------------------------------------
# Config keys.

@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stcfg") / "search_threads_config_dump")
    libdir = os.path.dirname(kc.LIB_PATH)  # linked as the katago program is (csrc/Makefile)
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe,
                    os.path.join(REPO, "tests", "helpers", "search_threads_config_dump.cpp"),
                    "-L" + libdir, "-lkatacoffee", "-Wl,-rpath," + libdir], check=True)

    def run(text, tmp_path):
        cfg = tmp_path / "c.cfg"
        cfg.write_text(text)
        r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, timeout=30)
        return r.returncode, [float(x) for x in r.stdout.split()], r.stderr
    return run


def test_config_keys_and_the_alias(dump, tmp_path):
    """The first pair is what `katago analysis` reads, the second what the other commands do:
    they ignore the keys (the reference's self-play and match configs carry numSearchThreads)."""
    off = [1.0, 1.0]
    assert dump("maxVisits = 50\n", tmp_path)[:2] == (0, off + off)  # absent: one playout a round
    assert dump("numSearchThreadsPerAnalysisThread = 16\n", tmp_path)[:2] == (0, [16.0, 1.0] + off)
    assert dump("numSearchThreads = 8\nnumVirtualLossesPerThread = 2.5\n", tmp_path)[:2] == (0, [8.0, 2.5] + off)
    # the full name wins over its alias
    assert dump("numSearchThreads = 8\nnumSearchThreadsPerAnalysisThread = 4\n", tmp_path)[:2] == (0, [4.0, 1.0] + off)
    text = open(os.path.join(REPO, "configs", "analysis_coffee5.cfg")).read()
    assert dump(text, tmp_path)[:2] == (0, off + off)  # the shipped config keeps it off
    assert "# numSearchThreadsPerAnalysisThread = 16" in text and "# numVirtualLossesPerThread" in text


BAD_KEYS = [("numSearchThreadsPerAnalysisThread", "0"), ("numSearchThreadsPerAnalysisThread", "33"),
            ("numSearchThreadsPerAnalysisThread", "four"), ("numSearchThreadsPerAnalysisThread", "2.5"),
            ("numSearchThreads", "0"), ("numSearchThreads", "64"), ("numSearchThreads", "-1"),
            ("numVirtualLossesPerThread", "0"), ("numVirtualLossesPerThread", "0.001"),
            ("numVirtualLossesPerThread", "1001"), ("numVirtualLossesPerThread", "nan"),
            ("numVirtualLossesPerThread", "1x")]


@pytest.mark.parametrize("key,value", BAD_KEYS, ids=["%s=%s" % b for b in BAD_KEYS])
def test_bad_config_values_are_refused_by_key(dump, tmp_path, key, value):
    rc, _, err = dump("%s = %s\n" % (key, value), tmp_path)
    assert rc == 1 and key in err, (rc, err)
    assert "other commands" not in err  # `katago analysis` alone reads the keys
