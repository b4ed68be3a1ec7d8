"""`katago analysis` with root restrictions: rootSymmetryPruning reports every
legal move of the empty board once, the pruned ones as copies of their orbit's survivor;
includePolicy, allowMoves / avoidMoves and their error lines."""
import json
import os
import subprocess

import pytest

import katacoffee_amd as kc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, A, P, VISITS = 5, 5, 25, 100, 64


def _pos(s):
    return (ord(s[2]) - 97) * A + (ord(s[1]) - 97) * X + (ord(s[0]) - 97)


def _service(lines, pruning):
    cmd = [os.path.join(REPO, "katacoffee_amd", "katago"), "analysis", "-config",
           os.path.join(REPO, "configs", "analysis_coffee5.cfg"), "-override-config",
           "maxVisits=%d,numAnalysisSlots=2,rootSymmetryPruning=%s" % (VISITS, "true" if pruning else "false")]
    r = subprocess.run(cmd, input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(line) for line in r.stdout.strip().split("\n")]
    assert len(out) == len(lines)
    return {o["id"]: o for o in out}


def test_pruned_session_reports_every_legal_move_once():
    out = _service(['{"id":"e","moves":[],"includePolicy":true}',
                    '{"id":"av","moves":[],"avoidMoves":[{"player":"B","moves":["cca"],"untilDepth":1}]}',
                    '{"id":"other","moves":[],"avoidMoves":[{"player":"W","moves":["cca"],"untilDepth":1}]}',
                    '{"id":"al","moves":[],"allowMoves":[{"player":"B","moves":["cca","aab"],"untilDepth":1}]}',
                    '{"id":"both","moves":[],"allowMoves":[{"player":"B","moves":["cca"],"untilDepth":1}],'
                    '"avoidMoves":[{"player":"B","moves":["ccb"],"untilDepth":1}]}',
                    '{"id":"deep","moves":[],"avoidMoves":[{"player":"B","moves":["cca"],"untilDepth":2}]}',
                    '{"id":"none","moves":["cca"],"allowMoves":[{"player":"W","moves":["cca"],"untilDepth":1}]}'],
                   pruning=True)
    o = out["e"]
    assert o["rootInfo"]["symmetries"] == list(range(8)) and o["rootInfo"]["visits"] == VISITS
    policy = o["policy"]
    assert len(policy) == P
    legal = [p for p in range(P) if policy[p] >= 0]
    assert len(legal) == 96 and all(policy[p] == -1 for p in range(P) if p not in legal)
    infos = o["moveInfos"]
    moves = [_pos(i["move"]) for i in infos]
    # every legal move once: the searched survivors, each with a child, and their copies
    survivors = {i["move"]: i for i in infos if "isSymmetryOf" not in i}
    copies = [i for i in infos if "isSymmetryOf" in i]
    assert copies and len(moves) == len(set(moves)) and set(moves) <= set(legal)
    orbit = lambda p: min(kc.symmetry_move(X, Y, s, p) for s in range(8))
    assert set(moves) == {p for p in legal if orbit(p) in {_pos(m) for m in survivors}}
    for mv in survivors:
        assert orbit(_pos(mv)) == _pos(mv)
    for c in copies:
        sv = survivors[c["isSymmetryOf"]]
        for key in ("visits", "winrate", "prior", "lcb", "order"):
            assert c[key] == sv[key], key
        src, dst = _pos(sv["move"]), _pos(c["move"])
        s = min(s for s in range(8) if kc.symmetry_move(X, Y, s, src) == dst)
        assert [_pos(m) for m in c["pv"]] == [kc.symmetry_move(X, Y, s, _pos(m)) for m in sv["pv"]]
        assert c["pv"][0] == c["move"]
    # an avoided move drops the transposes (cca is the centre's N move) and gets no entry
    av = out["av"]
    assert av["rootInfo"]["symmetries"] == [0, 1, 2, 3] and "policy" not in av
    assert _pos("cca") not in [_pos(i["move"]) for i in av["moveInfos"]]
    # an entry for the player who is not to move has no effect
    assert out["other"]["rootInfo"]["symmetries"] == list(range(8))
    assert len(out["other"]["moveInfos"]) > len([i for i in out["other"]["moveInfos"] if "isSymmetryOf" not in i])
    al = [_pos(i["move"]) for i in out["al"]["moveInfos"]]
    assert al and set(al) <= {_pos("cca"), _pos("aab")} and out["al"]["rootInfo"]["visits"] == VISITS
    assert out["both"]["field"] == "allowMoves" and "error" in out["both"]
    assert out["deep"]["field"] == "untilDepth" and "untilDepth" in out["deep"]["error"]
    assert out["none"]["field"] == "allowMoves" and "no legal move" in out["none"]["error"]


def test_without_pruning_there_are_no_copies():
    out = _service(['{"id":1,"moves":[],"includePolicy":true}', '{"id":2,"moves":[],"includePolicy":false}'],
                   pruning=False)
    assert all("isSymmetryOf" not in i for i in out[1]["moveInfos"]) and len(out[1]["policy"]) == P
    assert out[1]["rootInfo"]["symmetries"] == list(range(8)) and "policy" not in out[2]
