"""`katago analysis` with parallel playouts per search: the config key reaches the
engine, every query gets exactly its visits, and with the key at 1 (or absent) the command prints
what it printed before the feature existed -- tests/golden/cli_search_threads_k1.jsonl, recorded
from the command of the commit before it."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "cli_search_threads_k1.jsonl")
# the first moves of the oracle self-play line the analysis tests cut their positions from (seed 11)
LINE = [79, 83, 95, 41, 93, 72]
KEYS = "maxVisits=64,numAnalysisSlots=4,nnCacheSizePowerOfTwo=10"


def _move_name(pos):
    cell, d = pos % 25, pos // 25
    return chr(97 + cell % 5) + chr(97 + cell // 5) + chr(97 + d)


QUERIES = "".join(json.dumps(dict(id="q%d" % i, moves=[_move_name(m) for m in LINE[:n]], maxVisits=v)) + "\n"
                  for i, (n, v) in enumerate([(0, 64), (2, 50), (6, 33)]))


def _run(extra):
    cmd = [os.path.join(REPO, "katacoffee_amd", "katago"), "analysis", "-config",
           os.path.join(REPO, "configs", "analysis_coffee5.cfg"), "-override-config", KEYS + extra]
    return subprocess.run(cmd, input=QUERIES, capture_output=True, text=True, timeout=120)


def test_four_search_threads_answer_with_the_exact_visits():
    r = _run(",numSearchThreadsPerAnalysisThread=4")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "4 search threads per slot" in r.stderr
    out = {o["id"]: o for o in map(json.loads, r.stdout.strip().splitlines())}
    assert {k: o["rootInfo"]["visits"] for k, o in out.items()} == {"q0": 64, "q1": 50, "q2": 33}
    for o in out.values():
        assert sum(i["visits"] for i in o["moveInfos"]) == o["rootInfo"]["visits"] - 1
    # a round of slots x threads rows must fit one network launch: a start-up error naming the key
    bad = _run(",numSearchThreads=32,numAnalysisSlots=4096")
    assert bad.returncode != 0 and "numSearchThreadsPerAnalysisThread" in bad.stderr and "batch cap" in bad.stderr
    bad = _run(",numSearchThreadsPerAnalysisThread=33")
    assert bad.returncode != 0 and "numSearchThreadsPerAnalysisThread" in bad.stderr


@pytest.mark.parametrize("extra", ["", ",numSearchThreadsPerAnalysisThread=1", ",numSearchThreads=1"],
                         ids=["absent", "one", "alias"])
def test_one_search_thread_prints_what_the_command_printed_before(extra):
    r = _run(extra)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "search threads" not in r.stderr
    assert sorted(r.stdout.strip().splitlines()) == sorted(open(GOLDEN).read().strip().splitlines())
