"""Where an evidence-feed job's arrays lie (mcevidence_amd/csrc/feed_layout.hpp: ``FeedArena`` / ``FeedPinned`` of capi_feed.hpp, ``PrefixArena`` /
``PrefixPinned`` of capi_prefix.hpp, each one row of ``WsPlan`` takes), on the CPU, as a stand-alone program built with
-fsanitize=address,undefined: tests/native/feed_layout_check.cpp has the grid (d in 1, 2, 63, 64, 127; n1 in 2, 40, 513; n2 in 0, 1, 30; kmax in
2, 3, 33; the certificate and the device eigen-solver off and on; one and two systems; B in 1, 3, 256 with equal neighbours), the assertions
(alignment, order, no overlap, room for the documented content, sizing pass == placing pass, lam | status side by side) and the pins: six
named tuples per arena whose dev_bytes, host_bytes and offsets are what the library's ``feed_plan`` / ``prefix_plan`` counted by hand at
f000f58 ("Certify the run-time k-NN certificate on wrong lists; fix three holes"), the last commit that did.  Here: it builds, runs clean
and has seen what it should; and the scheme has one home."""
import os
import re
import subprocess

import pytest

from helpers import REPO

CSRC = os.path.join(REPO, "mcevidence_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("feed_layout") / "feed_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(REPO, "tests", "native", "feed_layout_check.cpp"), "-o", exe])
    return exe


def test_arenas_and_pinned_blocks_hold_on_the_grid_and_at_the_pins(checker):
    out = subprocess.run([checker, "all"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.fullmatch(r"ok feed=(\d+) prefix=(\d+) pins=(\d+)", out.stdout.strip().splitlines()[-1])
    assert m, out.stdout[-2000:]
    feed, prefix, pins = (int(v) for v in m.groups())
    # 5 * 3 * 3 * 3 * 2 * 2 = 540 grid points: one system without s2, one and two with it (540 * 5 / 3 feed arenas); B in 1, 3, 256, with the
    # prefixes' own systems on and off without s2 (540 * 3 * 4 / 3 prefix arenas); every pin passes through the grid's checks as well
    assert pins == 12 and feed == 900 + 6 and prefix == 2160 + 6


def test_the_checker_includes_only_the_layout_header():
    src = open(os.path.join(REPO, "tests", "native", "feed_layout_check.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["feed_layout.hpp"]
    for f in ("feed_layout.hpp", "ws_plan.hpp"):          # host only: nothing of HIP, nothing of the library's other headers
        text = open(os.path.join(CSRC, f)).read()
        assert not re.search(r"#include <hip|\bhip[A-Z]\w+|__global__|__device__", text) and set(re.findall(r'#include "([^"]+)"', text)) <= {"ws_plan.hpp"}, f


def test_the_scheme_has_one_home():
    """no hand-counted offset is left in the two jobs; the planner, the arena's guard and the per-device threads are each defined once"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip"))}
    for f in ("capi_feed.hpp", "capi_prefix.hpp"):
        assert not re.search(r"o_\w+ = off", src[f]) and "reinterpret_cast<double*>(dbase" not in src[f] and "align_up(" not in src[f], f
    assert [f for f, s in src.items() if re.search(r"struct WsPlan\b", s)] == ["ws_plan.hpp"]
    assert [f for f, s in src.items() if re.search(r"size_t prep_align\(", s)] == ["ws_plan.hpp"]
    assert [(f, len(re.findall(r"struct Quiesce\b", s))) for f, s in src.items() if "struct Quiesce" in s] == [("capi_feed.hpp", 1)]
    assert [(f, s.count("std::vector<std::thread>")) for f, s in src.items() if "std::thread" in s] == [("capi_feed.hpp", 1)]
    assert [(f, s.count("t_opt = inherited")) for f, s in src.items() if "t_opt = inherited" in s] == [("capi_feed.hpp", 1)]
    # the stages the two jobs share are the feed's: prefix defines none of its own
    for name in ("feed_check", "feed_copy_in", "feed_solve_host", "feed_eig_results", "feed_verify_enqueue"):
        assert len(re.findall(r"^int %s\(" % name, src["capi_feed.hpp"], re.M)) == 1 and name in src["capi_prefix.hpp"], name
    assert "hipMemcpy2D" not in src["capi_prefix.hpp"] and "mce_verify_knn_f64_dev" not in src["capi_prefix.hpp"]
    assert src["capi_feed.hpp"].count("hipMemcpy2DAsync(") == 2 and src["capi_feed.hpp"].count("hipMemcpy2D(") == 2
