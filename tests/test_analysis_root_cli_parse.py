"""The root keys of a `katago analysis` query (cli_analysis_query.h over cli_json.h) and the
shared rule (rootmask.h), compiled alone with tests/helpers/root_mask_san.cpp under
AddressSanitizer and UndefinedBehaviorSanitizer (host code only, no device): the new keys
parse, the bad forms are rejected naming their field, and the sanitized rule agrees with the
library's on the positions of tests/test_root_mask.py while the run stays clean."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import katacoffee_amd as kc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "katacoffee_amd", "csrc")
_spec = importlib.util.spec_from_file_location("root_mask_cases",
                                               os.path.join(REPO, "tests", "helpers", "root_mask_cases.py"))
rc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rc)

ENTRY = '{"player":"%s","moves":[%s],"untilDepth":%s}'


def _pos(s, X=5, A=25):
    return (ord(s[2]) - 97) * A + (ord(s[1]) - 97) * X + (ord(s[0]) - 97)


def _words(moves):
    return " ".join("%x" % w for w in kc.move_bits([_pos(m) for m in moves], kc.ANALYSIS_RESTRICT_WORDS))


GOOD = [
    ('{"id":1,"moves":[]}', "ok 0 0 " + _words([])),
    ('{"id":1,"includePolicy":true}', "ok 1 0 " + _words([])),
    ('{"id":1,"includePolicy":false,"avoidMoves":[]}', "ok 0 0 " + _words([])),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("B", '"cca","aab"', 1)), "ok 0 1 " + _words(["cca", "aab"])),
    ('{"id":1,"avoidMoves":[%s,%s]}' % (ENTRY % ("b", '"cca"', 1), ENTRY % ("B", '"eed"', 1)),
     "ok 0 1 " + _words(["cca", "eed"])),
    # an entry for the player who is not to move has no effect
    ('{"id":1,"avoidMoves":[%s,%s]}' % (ENTRY % ("W", '"cca"', 1), ENTRY % ("B", '"eed"', 1)), "ok 0 1 " + _words(["eed"])),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("W", '"cca"', 1)), "ok 0 0 " + _words([])),
    ('{"id":1,"allowMoves":[%s]}' % (ENTRY % ("B", '"cca"', 1)), "ok 0 2 " + _words(["cca"])),
    ('{"id":1,"allowMoves":[%s]}' % (ENTRY % ("W", '"cca"', 1)), "ok 0 0 " + _words([])),
    ('{ "id":1, "allowMoves" : [ { "untilDepth" : 1 , "moves":[ ], "player":"B" } ] }', "ok 0 2 " + _words([])),
]
BAD = [
    ('{"id":1,"allowMoves":[%s],"avoidMoves":[%s]}' % (ENTRY % ("B", '"cca"', 1), ENTRY % ("B", '"ccb"', 1)), "allowMoves"),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("B", '"cca"', 2)), "untilDepth"),
    ('{"id":1,"allowMoves":[%s]}' % (ENTRY % ("B", '"cca"', 0)), "untilDepth"),
    ('{"id":1,"avoidMoves":[{"player":"B","moves":["cca"]}]}', "untilDepth"),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("B", '"cca"', '"1"')), "untilDepth"),
    ('{"id":1,"allowMoves":[%s,%s]}' % (ENTRY % ("B", '"cca"', 1), ENTRY % ("B", '"ccb"', 1)), "allowMoves"),
    ('{"id":1,"allowMoves":[]}', "allowMoves"),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("X", '"cca"', 1)), "avoidMoves"),
    ('{"id":1,"avoidMoves":[{"moves":["cca"],"untilDepth":1}]}', "avoidMoves"),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("B", '"zzz"', 1)), "avoidMoves"),
    ('{"id":1,"avoidMoves":[%s]}' % (ENTRY % ("B", '"cce"', 1)), "avoidMoves"),
    ('{"id":1,"avoidMoves":["cca"]}', "json"),
    ('{"id":1,"avoidMoves":{"player":"B"}}', "json"),
    ('{"id":1,"avoidMoves":[{"player":{"a":1}}]}', "json"),
    ('{"id":1,"avoidMoves":[{"player":"B","moves":[["cca"]],"untilDepth":1}]}', "json"),
    ('{"id":1,"avoidMoves":[{"player":"B","moves":["cca"],"untilDepth":1}', "json"),
    ('{"id":1,"avoidMoves":[{"player":"B","player":"W"}]}', "json"),
    ('{"id":1,"avoidMoves":[' + '{"a":' * 3000, "json"),
    ('{"id":1,"includePolicy":1}', "includePolicy"),
    ('{"id":1,"includePolicy":"true"}', "includePolicy"),
    ('{"id":1,"includePolicy":tru}', "json"),
    ('{"id":true}', "json"),
    ('{"id":1,"moves":[{"player":"B"}]}', "json"),
]


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp("rootsan") / "root_mask_san")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(REPO, "tests", "helpers", "root_mask_san.cpp"),
                    "-o", exe], check=True)
    return exe


def _run(exe, lines):
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stderr == b"", p.stderr.decode(errors="replace")[-2000:]  # no sanitizer report
    out = p.stdout.decode().split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def test_root_keys_parse(san):
    out = _run(san, ["Q 5 5 1 " + q for q, _ in GOOD])
    assert out == [want for _, want in GOOD]
    # a 10x10 board's positions do not fit the set
    out = _run(san, ["Q 10 10 1 " + GOOD[3][0]])
    assert out[0].startswith("error avoidMoves|")


def test_bad_root_keys_name_their_field(san):
    out = _run(san, ["Q 5 5 1 " + q for q, _ in BAD])
    for (q, field), got in zip(BAD, out):
        assert got.startswith("error %s|" % field) and len(got) > len("error %s|" % field), (q[:80], got)


def test_sanitized_rule_equals_the_library(san):
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    lines, want = [], []
    for _, X, Y, W, moves in rc.cases():
        P = 4 * X * Y
        for kw in ({}, {"avoid": [0, 7]}, {"allow": [1, 2, X * Y + 3]}, {"prune": False}):
            e = rc.expected(X, Y, W, moves, avoid=kw.get("avoid"), allow=kw.get("allow"), prune=kw.get("prune", True))
            col, hc, hd = rc.library_inputs(e["board"], e["hist"])
            r = kc.root_mask(X, Y, W, col, hc, hd, e["legal"], avoid_moves=kw.get("avoid"), allow_moves=kw.get("allow"),
                             prune=kw.get("prune", True))
            np.testing.assert_array_equal(r["mask"], e["mask"])
            mode = 1 if "avoid" in kw else (2 if "allow" in kw else 0)
            legal = kc.move_bits(np.nonzero(e["legal"])[0], (P + 31) // 32)
            avoid = kc.move_bits(kw.get("avoid", kw.get("allow", [])), kc.ANALYSIS_RESTRICT_WORDS)
            hist = " ".join("%d %d" % (c, d) for c, d in e["hist"])
            lines.append("M %d %d %d %d %d %s %s %s %s" % (
                X, Y, int(kw.get("prune", True)), mode, len(e["hist"]), hist, "".join(str(c) for c in e["board"].cells),
                " ".join("%x" % w for w in legal), " ".join("%x" % w for w in avoid)))
            mask = kc.move_bits(np.nonzero(r["mask"])[0], (P + 31) // 32)
            want.append("mask %s syms %d masked %d left %d" % (" ".join("%x" % w for w in mask), r["bits"],
                                                              r["num_masked"], r["left"]))
    assert _run(san, lines) == want
