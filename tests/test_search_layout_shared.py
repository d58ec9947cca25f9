"""Where the arrays of one nearest-neighbour search lie (mcevidence_amd/csrc/search_layout.hpp: ``PruneArena``, ``SymArena``, ``SearchArena`` in its
four shapes, ``PairsOnceArena``, each a row of ``WsPlan`` takes), on the CPU, as a stand-alone program built with
-fsanitize=address,undefined: tests/native/search_layout_check.cpp has the grid (every family; d in 1, 2, 15, 16, 63, 64, 127, 128, 1024; nq, nr
in 1, 31, 32, 513, 70 000; K in 1, 4, 16, 17, 32, 33; pruned walk, heavy waves and symmetric sweep off and on; S in 1, 3), the assertions
(alignment, order, no overlap, room for the documented content, sizing pass == placing pass, the three counters contiguous, cf32 inside Xs
exactly when the rule says so) and reads the pins: tests/golden/search_layout_pins.txt, twenty plans whose total and every offset are
what ``make_plan`` / ``prune_layout`` / ``sym_layout`` / ``pairs_once_shape`` counted by hand at 3aad787 ("One table of posterior statistics for
host, resident and farm routes"), the last commit that did, with the rocPRIM sizes that library saw as inputs.  Here: it builds, runs
clean and has seen what it should; and the scheme has one home."""
import os
import re
import subprocess

import pytest

from helpers import REPO

CSRC = os.path.join(REPO, "mcevidence_amd", "csrc")
PINS = os.path.join(REPO, "tests", "golden", "search_layout_pins.txt")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_layout") / "search_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(REPO, "tests", "native", "search_layout_check.cpp"), "-o", exe])
    return exe


def test_arenas_hold_on_the_grid_and_at_the_pins(checker):
    out = subprocess.run([checker, PINS], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.fullmatch(r"ok grid=(\d+) pins=(\d+)", out.stdout.strip().splitlines()[-1])
    assert m, out.stdout[-2000:]
    grid, pins = (int(v) for v in m.groups())
    # 9 * 5 * 5 * 6 = 1350 points per family: three families of one shape, the filter in four (plain, pruned, pruned with heavy waves,
    # symmetric -- the last also as a pairs-once share with S = 1 and 3); every pin passes through the grid's checks as well
    assert grid == 1350 * (3 + 4 + 2) and pins == 20
    names = [line.split()[1] for line in open(PINS) if line.startswith("PIN ")]
    assert len(names) == len(set(names)) == 20


def test_a_moved_array_fails_a_pin(checker, tmp_path):
    """the pins bite: the same file with one offset moved by an alignment unit is refused"""
    text = open(PINS).read()
    assert " thr=16242432 " in text
    bad = tmp_path / "pins.txt"
    bad.write_text(text.replace(" thr=16242432 ", " thr=16242688 "))
    out = subprocess.run([checker, str(bad)], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "thr" in out.stderr


def test_the_checker_includes_only_the_layout_header():
    src = open(os.path.join(REPO, "tests", "native", "search_layout_check.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["search_layout.hpp"]
    for f in ("search_layout.hpp", "ws_plan.hpp"):          # host only: nothing of HIP, nothing of the library's other headers
        text = open(os.path.join(CSRC, f)).read()
        assert not re.search(r"#include <hip|\bhip[A-Z]\w+|__global__|__device__|_Float16 \*|rocprim::", text) and set(re.findall(r'#include "([^"]+)"', text)) <= {"ws_plan.hpp"}, f


def test_the_scheme_has_one_home():
    """no hand-counted offset is left in the search: the planner's fields, the two layout structs and the cast blocks are gone"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip"))}
    for f, s in src.items():
        assert "ws + p.off_" not in s and not re.search(r"reinterpret_cast<[^>]+>\(ws \+ L\.", s) and not re.search(r"\bp\.off_\w+|\bp\.[ps]l\.", s), f
        assert not re.search(r"\b(PruneLayout|SymLayout|prune_layout|sym_layout)\b", s), f
    assert [f for f, s in src.items() if re.search(r"struct WsPlan\b", s)] == ["ws_plan.hpp"]
    for name in ("PruneArena", "SymArena", "SearchArena", "PairsOnceArena", "SearchSizes"):
        assert [f for f, s in src.items() if re.search(r"struct %s\b" % name, s)] == ["search_layout.hpp"], name
    # align_up stays only where it is not a layout: the reduction's scratch size
    for f in ("capi_search.hpp", "capi_apo.hpp", "prune.hip", "prune.hpp", "search_layout.hpp"):
        assert "align_up(" not in src[f], f
    assert len(re.findall(r"\balign_up\(", src["capi_plan.hpp"])) == 2 and re.search(r"size_t dotp_ws_bytes\([^)]*\)\n\{[^}]*align_up\(", src["capi_plan.hpp"])
    # the rocPRIM size queries stay with the sorts they serve, one small function each
    for name in ("prune_tmp_bytes", "sym_tmp_bytes"):
        assert len(re.findall(r"^size_t %s\(" % name, src["prune.hip"], re.M)) == 1 and len(re.findall(r"mce::%s\(" % name, src["capi_plan.hpp"])) == 1, name
    # make_plan in steps: no function of the planner is longer than about 80 lines
    lines = src["capi_plan.hpp"].splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"^[A-Za-z].*\)$", l) and i + 1 < len(lines) and lines[i + 1] == "{"]
    assert len(starts) >= 12
    for i in starts:
        assert lines.index("}", i) - i <= 85, lines[i]
