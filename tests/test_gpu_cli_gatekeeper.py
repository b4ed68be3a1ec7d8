"""`katago gatekeeper` (the process boundary of match play, command/gatekeeper.cpp): a fresh
child process gates a candidate net against an accepted one on the GPU; the verdict, the
model file's move and the .sgfs are read back."""
import glob
import os
import re
import subprocess
import time

import numpy as np
import pytest

import katacoffee_amd as kc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, W, N, G = 5, 5, 4, 8, 8
MOVE = re.compile(r";([BW])\[([a-z])([a-z])([a-d])\]")


def _gate(tmp_path, extra=()):
    d = {k: tmp_path / k for k in ("test", "accepted", "rejected", "sgf", "selfplay")}
    cmd = [os.path.join(REPO, "katacoffee_amd", "katago"), "gatekeeper", "-config",
           os.path.join(REPO, "configs", "gatekeeper_coffee5.cfg"), "-test-models-dir", str(d["test"]),
           "-accepted-models-dir", str(d["accepted"]), "-rejected-models-dir", str(d["rejected"]),
           "-sgf-output-dir", str(d["sgf"]), "-selfplay-dir", str(d["selfplay"]), "-quit-if-no-nets-to-test",
           "-override-config", "numGamesPerGating=%d,numGameThreads=%d,maxVisits=8,allowResignation=true" % (N, G)]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300)
    return r, d


def _names(dirpath):
    return sorted(os.listdir(dirpath)) if os.path.isdir(dirpath) else []


def _replay_sgf(line):
    """Replays one SGF line on the device rules: every move legal, colours alternating from
    black; returns (finished, winner)."""
    A = X * Y
    cells = np.zeros((1, A), np.uint8)
    lc, ld, pla = np.array([-1], np.int8), np.array([4], np.int8), 1
    fin = win = 0
    for colour, cx, cy, cd in MOVE.findall(line):
        assert fin == 0 and colour == "BW"[pla - 1]
        cell, dr = (ord(cy) - 97) * X + (ord(cx) - 97), ord(cd) - 97
        legal, _ = kc.rules_batch(X, Y, W, cells, lc, ld, np.array([pla], np.uint8))
        assert legal[0, dr * A + cell] == 1, line
        cells, f, w, _, _, _ = kc.play_batch(X, Y, W, cells, lc, ld, np.array([pla], np.uint8),
                                             np.array([dr * A + cell], np.int32))
        fin, win = int(f[0]), int(w[0])
        lc, ld, pla = np.array([cell], np.int8), np.array([dr], np.int8), 3 - pla
    return fin, win


def test_gatekeeper_gates_and_autorejects(tmp_path):
    for k in ("test", "accepted"):
        (tmp_path / k).mkdir()
    kc.write_random_model("b2c32", 21, str(tmp_path / "accepted" / "base-s0.cfnn"))
    kc.write_random_model("b2c32", 22, str(tmp_path / "test" / "cand-s1.cfnn"))
    now = time.time()
    os.utime(tmp_path / "accepted" / "base-s0.cfnn", (now - 100, now - 100))
    os.utime(tmp_path / "test" / "cand-s1.cfnn", (now - 50, now - 50))
    r, d = _gate(tmp_path)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log
    assert log.count("allowResignation") == 1  # noted once: the games are played out
    # the verdict line, and the file in exactly one of the two directories, agreeing with it
    m = re.search(r"candidate cand-s1 (accepted|rejected): score ([0-9.]+) to ([0-9.]+) in (\d+) games", log)
    assert m, log
    verdict, cand, base, games = m.group(1), float(m.group(2)), float(m.group(3)), int(m.group(4))
    assert verdict == ("rejected" if base > cand else "accepted")  # the candidate wins ties
    assert cand + base == games <= N
    assert _names(d["test"]) == []
    in_acc, in_rej = "cand-s1.cfnn" in _names(d["accepted"]), "cand-s1.cfnn" in _names(d["rejected"])
    assert in_acc != in_rej and in_acc == (verdict == "accepted")
    if in_acc:
        assert _names(d["selfplay"] / "cand-s1") == ["sgfs", "tdata", "vadata"]
    # the counted games, in tally order, with the colours of the rule (slot s, game 0 since
    # N == G: the candidate is black iff s is even)
    files = glob.glob(str(d["sgf"] / "cand-s1" / "*.sgfs"))
    assert len(files) == 1
    lines = open(files[0]).read().splitlines()
    assert len(lines) == games
    pts = {"cand-s1": 0.0, "base-s0": 0.0}
    slots = set()
    for line in lines:
        pb, pw = re.search(r"PB\[([^\]]*)\]", line).group(1), re.search(r"PW\[([^\]]*)\]", line).group(1)
        slot, num = map(int, re.search(r"gameId=(\d+):(\d+)", line).groups())
        assert num * G + slot < N and slot not in slots
        slots.add(slot)
        assert (pb, pw) == (("cand-s1", "base-s0") if (slot + num) % 2 == 0 else ("base-s0", "cand-s1"))
        res = re.search(r"RE\[([^\]]*)\]", line).group(1)
        fin, win = _replay_sgf(line)
        assert (fin, win) == {"B+": (1, 1), "W+": (1, 2)}.get(res, (fin, 0))
        if res == "0":
            pts[pb] += 0.5
            pts[pw] += 0.5
        else:
            pts[pb if res == "B+" else pw] += 1.0
    assert (pts["cand-s1"], pts["base-s0"]) == (cand, base)
    # a candidate older than the newest accepted model is rejected without a game
    kc.write_random_model("b2c32", 23, str(tmp_path / "test" / "old-s2.cfnn"))
    os.utime(tmp_path / "test" / "old-s2.cfnn", (now - 500, now - 500))
    r2, _ = _gate(tmp_path)
    log2 = r2.stdout + r2.stderr
    assert r2.returncode == 0, log2
    assert "rejected without playing" in log2 and "score" not in log2
    assert "old-s2.cfnn" in _names(d["rejected"]) and _names(d["test"]) == []
    assert not os.path.isdir(d["sgf"] / "old-s2")


def test_unknown_subcommand_keeps_the_usage_error():
    r = subprocess.run([os.path.join(REPO, "katacoffee_amd", "katago"), "match"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: katago selfplay" in r.stderr
