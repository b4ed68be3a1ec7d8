"""The JSON reader of `katago analysis` (katacoffee_amd/csrc/cli_json.h), compiled alone with
a small main under AddressSanitizer and UndefinedBehaviorSanitizer (host code only): good
lines parse, and truncated, deeply nested, over-long and non-UTF-8 lines are each rejected
with a message while the run stays clean."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(REPO, "katacoffee_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "cli_json.h"
int main() {
  std::string line;
  while(std::getline(std::cin, line)) {
    kcjson::Object o;
    std::string err;
    if(kcjson::parseLine(line, o, err)) {
      printf("ok %zu", o.fields.size());
      for(const auto& f : o.fields) {
        const kcjson::Value& v = f.second;
        if(v.kind == kcjson::Value::INT) printf(" %s=%lld", f.first.c_str(), v.i);
        else if(v.kind == kcjson::Value::STRING) printf(" %s=%s", f.first.c_str(), kcjson::quote(v.s).c_str());
        else printf(" %s=[%zu]", f.first.c_str(), v.a.size());
      }
      printf("\n");
    } else {
      printf("error %s\n", err.c_str());
    }
  }
  return 0;
}
"""

GOOD = [
    (b'{"id":"q1","moves":["ccb","bca"],"maxVisits":50}', 'ok 3 id="q1" moves=[2] maxVisits=50'),
    (b'  { "id" : 7 , "moves" : [ ] }  ', "ok 2 id=7 moves=[0]"),
    (b"{}", "ok 0"),
    (b'{"id":"\\u00e9\\ud83d\\ude00\\n","n":-12}', 'ok 2 id="é\U0001F600\\u000a" n=-12'),
    ('{"id":"café"}'.encode("utf-8"), 'ok 1 id="café"'),
]
FULL = b'{"id":"q1","moves":["ccb","bca"],"maxVisits":50}'
BAD = (
    # every truncation of a good line
    [(FULL[:n], None) for n in range(len(FULL))]
    + [
        (b"[" * 5000, "expected '{'"),
        (b'{"a":' + b"[" * 5000, "nested arrays"),
        (b'{"a":' * 3000, "nested objects"),
        (b'{"a":[' + b'["x"],' * 10 + b"]}", "nested arrays"),
        (b'{"id":"' + b"x" * 70000 + b'"}', "longer than"),
        (b'{"id":"' + b"x" * 5000 + b'"}', "string too long"),
        (b'{"moves":[' + b'"aaa",' * 1100 + b'"aaa"]}', "array too long"),
        (b'{"id":"\xff\xfe"}', "UTF-8"),
        (b'{"id":"\xc3"}', "UTF-8"),
        (b'{"id":"\xc0\xaf"}', "UTF-8"),          # overlong
        (b'{"id":"\xed\xa0\x80"}', "UTF-8"),      # a surrogate
        (b'{"id":"\xf4\x90\x80\x80"}', "UTF-8"),  # past U+10FFFF
        (b'{"id":"\xe2\x82"}', "UTF-8"),
        (b'{"id":"\\ud800"}', "surrogate"),
        (b'{"id":"\\u12"}', "escape"),
        (b'{"id":"a\x01b"}', "control character"),
        (b'{"id":1.5}', "only integers"),
        (b'{"id":99999999999999999999}', "out of range"),
        (b'{"id":true}', "expected a string"),
        (b'{"id":"a","id":"b"}', "duplicate key"),
        (b'{"id":"a"} x', "text after"),
        (b'{"id" "a"}', "expected ':'"),
        (b'{"id":01}', "leading zero"),
    ]
)


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the JSON reader"
    d = tmp_path_factory.mktemp("json")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = str(d / "json_reader")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", HEADER_DIR, str(src), "-o", exe], check=True)
    return exe


def _run(exe, lines):
    for line in lines:
        assert b"\n" not in line
    p = subprocess.run([exe], input=b"\n".join(lines) + b"\n", capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stderr == b"", p.stderr.decode(errors="replace")[-2000:]  # no sanitizer report
    out = p.stdout.decode("utf-8").split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def test_good_lines_parse(reader):
    out = _run(reader, [g for g, _ in GOOD])
    assert out == [want for _, want in GOOD]


def test_bad_lines_are_rejected_with_a_message(reader):
    out = _run(reader, [b for b, _ in BAD])
    for (line, word), got in zip(BAD, out):
        assert got.startswith("error ") and len(got) > len("error "), (line[:60], got)
        if word is not None:
            assert word in got, (line[:60], got)
