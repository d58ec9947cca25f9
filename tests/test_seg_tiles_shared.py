"""The segment-tile scheme on the CPU (mcevidence_amd/csrc/seg_tiles.hpp: the table builder, the tile lookup and the keyed search that the
per-system statistics kernels and the host side of the library share), as a stand-alone program built with
-fsanitize=address,undefined: tests/native/seg_tiles_check.cpp has the cases and the assertions (segment lists drawn from the row counts
0, 1, 511, 512, 513, 1024, 1025, 4100 with empty segments first, in the middle, last, side by side and alone; every tile against a
direct count; the keyed search against a scan; the refusal at 2^31 tiles).  Here: it builds, runs clean and has seen what it should."""
import os
import re
import subprocess

import pytest

from helpers import REPO

CSRC = os.path.join(REPO, "mcevidence_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_tiles") / "seg_tiles_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(REPO, "tests", "native", "seg_tiles_check.cpp"), "-o", exe])
    return exe


def test_table_lookup_and_search_hold_on_every_list(checker):
    out = subprocess.run([checker, "all"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.fullmatch(r"ok lists=(\d+) tiles=(\d+) keys=(\d+)", out.stdout.strip().splitlines()[-1])
    assert m, out.stdout[-2000:]
    lists, tiles, keys = (int(v) for v in m.groups())
    # 8 + 64 + 512 lists of one to three segments and 11 named ones; a list of all eight counts alone has 1+1+1+2+2+3+9 = 19 tiles
    assert lists == 8 + 64 + 512 + 11 and tiles > 19 * 2 and keys > lists


def test_the_scheme_has_one_home():
    """the tile size, the search loop and block_sum are each defined once; no statistics kernel header goes through reduce_kernels.hpp"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip"))}
    assert [f for f, s in src.items() if re.search(r"double block_sum\(", s)] == ["block_reduce.hpp"]
    assert [f for f, s in src.items() if re.search(r"if \([^;]*<= \w+\) lo = mid;", s)] == ["seg_tiles.hpp"]
    assert [f for f, s in src.items() if re.search(r"TileRows = 512\b", s)] == ["seg_tiles.hpp"]
    assert not [f for f, s in src.items() if f.startswith("capi") and "auto take = [&]" in s]            # (WsPlan declares a workspace)
    for f in ("like_moments_kernels.hpp", "jack_group_kernels.hpp", "param_summary_kernels.hpp", "jack_kernels.hpp", "prefix_kernels.hpp"):
        assert '#include "reduce_kernels.hpp"' not in src[f] and '#include "block_reduce.hpp"' in src[f], f
