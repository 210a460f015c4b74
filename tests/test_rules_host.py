"""The warm-up window schedule of csrc/potus_rules.hpp, without a GPU.

The header states windowed_adaptation's rules once for the device samplers and for the host's dense schedule; it compiles with a
plain C++ compiler.  A stand-alone program drives the rules the way their callers do -- potus_create's buffer adjustment, then one
rule_window_flags per warm-up iteration and one rule_next_window per window end -- and prints the windows; they must be exactly
those of tests/adaptation_replay.window_schedule, the restatement the GPU replay tests check the device against.  (The cluster sampler
keeps its own two lines of the window flags, potus_cluster.hpp::cl_adapt_after_transition: those are covered by the GPU replay only.)"""
import shutil
import subprocess
from pathlib import Path

import pytest

from adaptation_replay import window_schedule

ROOT = Path(__file__).resolve().parent.parent

PROGRAM = r"""
#include "potus_rules.hpp"
#include <cstdio>
#include <cstdlib>
// argv: groups of num_warmup init_buffer term_buffer window (raw options); a line per group: the adjusted buffers, then first-last of every window
int main(int argc, char **argv) {
  for (int a = 1; a + 3 < argc; a += 4) {
    const int nw = atoi(argv[a]);
    int ib = atoi(argv[a + 1]), tb = atoi(argv[a + 2]), bw = atoi(argv[a + 3]);
    rule_window_params(nw, ib, tb, bw);
    int win_next = rule_first_window_end(ib, bw), win_size = bw, first = -1;
    printf("%d %d %d:", ib, tb, bw);
    for (int wc = 0; wc < nw; wc++) {                   // the chain's win_counter: one per warm-up transition
      int in_window, end_window;
      rule_window_flags(nw, ib, tb, wc, win_next, in_window, end_window);
      if (in_window && first < 0) first = wc;
      if (end_window) {
        printf(" %d-%d", first, wc);
        first = -1;
        rule_next_window(nw, tb, wc, win_next, win_size);
      }
    }
    printf("\n");
  }
  return 0;
}
"""

WARMUPS = (19, 20, 21, 50, 150, 500, 1000)
# (init_buffer, term_buffer, window): Stan's defaults (with them 500 is the reference's 75 | 25, 50, 100, 200 | 50, and every warm-up
# below 150 takes the 15 % / 10 % adjustment); buffers that fit from 50 on; buffers that need the adjustment up to 249
BUFFERS = ((75, 50, 25), (10, 5, 20), (100, 50, 100))
CASES = [(nw, *b) for b in BUFFERS for nw in WARMUPS] + [(30, 75, 50, 25)]


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile potus_rules.hpp on its own"
    tmp = tmp_path_factory.mktemp("rules")
    (tmp / "rules_main.cpp").write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "us_potus_model_amd" / "csrc"), str(tmp / "rules_main.cpp"),
                    "-o", str(tmp / "rules_main")], check=True)
    out = subprocess.run([str(tmp / "rules_main"), *[str(v) for c in CASES for v in c]], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(CASES)
    got = {}
    for case, line in zip(CASES, out):
        head, _, tail = line.partition(":")
        got[case] = (tuple(int(v) for v in head.split()), [tuple(int(v) for v in w.split("-")) for w in tail.split()])
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_window_ends_are_those_of_the_replay(schedules, case):
    nw, ib, tb, bw = case
    assert schedules[case][1] == window_schedule(nw, ib, tb, bw)


def test_the_cases_cover_what_they_are_meant_to(schedules):
    assert schedules[(500, 75, 50, 25)] == ((75, 50, 25), [(75, 99), (100, 149), (150, 249), (250, 449)])   # the reference's schedule
    assert schedules[(19, 75, 50, 25)] == ((75, 50, 25), [])                                                # no windows below 20, buffers as given
    assert schedules[(30, 75, 50, 25)] == ((4, 3, 23), [(4, 26)])                                           # adjusted to 4 | 23 | 3
    assert schedules[(150, 75, 50, 25)][0] == (75, 50, 25) and schedules[(50, 75, 50, 25)][0] == (7, 5, 38)  # exactly fitting / adjusted
    assert schedules[(150, 100, 50, 100)][0] == (22, 15, 113) and schedules[(500, 100, 50, 100)][0] == (100, 50, 100)
    assert any(len(w) > 1 for _, w in schedules.values()) and any(len(w) == 1 for _, w in schedules.values())
