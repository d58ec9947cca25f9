"""The search planner sizes its workspace as ONE typed row (csrc/search_layout.hpp: ``SearchArena``; capi_plan.hpp: ``plan_sizes``): what must
not have moved when make_plan's three hand-counted layouts went.  The sizes are those that the library built at 3aad787 ("One table of
posterior statistics for host, resident and farm routes") planned, the last commit whose planner counted by hand.  Workspace queries do no
device work, so this is no GPU test.  Plans with the pruned walk's or the symmetric sweep's scratch hold rocPRIM's answer for its temporary
storage and are compared old against new instead (tools/search_sizes.py; docs/design/search_layout.md) -- here only what does not depend on
it: the symmetric scratch is reserved exactly when the caller does not rule it out, and a pairs-once share adds the same bytes to it."""
import pytest

from mcevidence_amd import _capi

Opt = _capi.Options

# (nq, nr, d, K), options -> workspace bytes
PLANNED = {
    "long rows, d = 300": ((513, 70000, 300, 4), {}, 183010048),
    "generic, K = 40": ((1000, 1000, 6, 40), {}, 811776),
    "fp64 sweep, wide form, d = 100": ((5000, 5000, 100, 4), dict(search_mode=1), 7874048),
    "fp64 sweep, d = 6, K = 17": ((31, 513, 6, 17), dict(search_mode=1), 665088),
    "deep filter, d = 100": ((20000, 20000, 100, 4), {}, 17024768),
    "deep filter, two passes": ((20000, 20000, 100, 20), {}, 58312448),
    "fp16 filter, KST = 1": ((5000, 70000, 6, 4), {}, 6833920),
    "fp16 filter, KST = 2": ((5000, 70000, 27, 9), {}, 17123072),
    "fp16 filter, KST = 3": ((5000, 70000, 45, 9), {}, 19498752),
    "fp16 filter, KST = 4": ((5000, 70000, 63, 16), {}, 24872704),
    "fp16 filter, two passes, K = 20": ((5000, 70000, 6, 20), {}, 18630400),
    "wide_ok: 489 blocks rounded up to 490": ((250001, 300000, 6, 4), dict(prune_mode=1, sym_mode=1), 34113280),
    "same_set = 0": ((1000000, 1000000, 27, 9), dict(same_set=0), 288540416),
    "sym off": ((1000000, 1000000, 27, 9), dict(sym_mode=1, same_set=1), 288540416),
}


@pytest.mark.parametrize("name", sorted(PLANNED))
def test_the_planner_sizes_what_it_sized_by_hand(name):
    shape, opt, planned = PLANNED[name]
    assert _capi.knn_workspace_bytes(*shape, options=Opt(**opt)) == planned
    if not opt:
        assert _capi.knn_workspace_bytes(*shape) == planned


def test_symmetric_scratch_is_reserved_unless_ruled_out_and_a_pairs_once_share_adds_what_it_added():
    shape = (1000000, 1000000, 27, 9)
    one, unknown, two = (_capi.knn_workspace_bytes(*shape, options=Opt(same_set=s)) for s in (1, -1, 0))
    assert one == unknown == _capi.knn_workspace_bytes(*shape) and two == 288540416
    # perm, keys_a, keys_b, vals_a, rrow (4 B a padded row), thr (8), rtile, Ys, slots [12], the counters, the buckets: all but rocPRIM's scratch
    assert one - two >= 1000448 * (4 * 5 + 8 + 12 * 8) + 1000448 // 32 * 4 + 1000000 * 27 * 8 + 1954 * 12 + 1954 * 39936 * 16
    # the reduction's partial sums + S = 2 (two ranks) or 8 (eight) list sets of [12][nq_pad] doubles and ints behind the search's arena
    assert _capi.pairs_once_workspace_bytes(1000000, 27, 10, 2) - one == 288441600
    assert _capi.pairs_once_workspace_bytes(1000000, 27, 10, 8) - one == 1008764160
    assert _capi.pairs_once_workspace_bytes(1000000, 27, 10, 1) == 0
