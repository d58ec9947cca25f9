"""posterior.py: the table of the statistics next to ln E, the farm's wave rule with a recording measure, and the host route looping over
the table in NumPy -- no device, no library."""
import numpy as np
import pytest

from helpers import OracleBackend
from mcevidence_amd import contours, covariance, information, marginals, posterior, summary
from mcevidence_amd.evidence import MCEvidence
from mcevidence_amd.synth import gaussian_chain


def _same(a, b):
    """bit for bit, through dicts, sequences and arrays"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and not isinstance(b, np.ndarray):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" and b.dtype.kind == "f":
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a.shape == b.shape and bool(np.all(a == b))


def test_the_table_is_the_five_statistics_in_logging_order():
    assert [st.key for st in posterior.STATS] == ["information", "summary", "marginals", "contours", "covariance"]
    assert [st.attr for st in posterior.STATS] == [None, "param_summary", "param_marginals", "param_contours", "param_cov"]
    assert posterior.BY_KEY["contours"] is posterior.CONTOURS and set(posterior.BY_KEY) == set(posterior.KEYS)


def test_per_root_is_the_farms_rule_for_every_statistic():
    per = posterior.SUMMARY.per_root
    assert per(None, 3) == [None] * 3 and per(True, 2) == [True, True]
    assert per((0.68, 0.95), 2) == [(0.68, 0.95)] * 2 and per([0.9, 0.5], 2) == [[0.9, 0.5]] * 2      # bare numbers: ONE value
    assert per([(0.9,), None], 2) == [(0.9,), None] and per([True, False, (0.5, 0.9)], 3) == [True, False, (0.5, 0.9)]
    with pytest.raises(ValueError, match="summary: expected 2 entries, got 3"):
        per([True, None, None], 2)
    with pytest.raises(ValueError, match=r"^summary=\[0\.5, None\]: either probabilities \(one value for every root\) or one entry per root \(None, True or a "
                                         r"sequence of probabilities each\), not a mixture$"):
        per([0.5, None], 2)
    for st in (posterior.MARGINALS, posterior.CONTOURS):           # (contours take the marginals' rule, with its words)
        per = st.per_root
        assert per(None, 3) == [None] * 3 and per({"grid": 64}, 2) == [{"grid": 64}] * 2
        assert per([0.9, 0.5], 2) == [[0.9, 0.5]] * 2 and per([(0.9,), None, {"grid": 64}], 3) == [(0.9,), None, {"grid": 64}]
        with pytest.raises(ValueError, match="marginals: expected 2 entries, got 3"):
            per([True, None, None], 2)
        with pytest.raises(ValueError, match=r"^marginals=\[0\.5, None\]: either one value for every root or one entry per root \(None, True, a sequence of "
                                             r"probabilities or a dict each\), not a mixture$"):
            per([0.5, None], 2)
    per = posterior.per_root_bounds
    assert per("ranges", 3) == ["ranges"] * 3 and per([(0, 1), (None, 2)], 2) == [[(0, 1), (None, 2)]] * 2
    assert per(["ranges", None, {"a": (0, 1)}], 3) == ["ranges", None, {"a": (0, 1)}] and per([[(0, 1)], None], 2) == [[(0, 1)], None]
    with pytest.raises(ValueError, match=r"^bounds=\['ranges', 3\.0\]: either one value for every root or one entry per root \(None, 'ranges', a mapping or a "
                                         r"sequence of \(lo, hi\) pairs each\), not a mixture$"):
        per(["ranges", 3.0], 2)
    for st in (posterior.INFORMATION, posterior.COVARIANCE):
        assert st.per_root(True, 2) == [True, True] and st.per_root([True, None], 2) == [True, None]
        with pytest.raises(ValueError, match="%s: expected 3 entries, got 2" % st.key):
            st.per_root([True, None], 3)


def test_resolve_is_none_when_unset_and_equal_for_equal_values():
    names = ["a", "b", "c"]
    for st in posterior.STATS:
        for unset in (None, False):
            assert st.resolve({st.key: unset}, names, 3, None) is None
    asks = {"information": (True, True), "summary": ((0.9, 0.5), [0.9, 0.5]), "covariance": (True, True),
            "marginals": ({"probs": (0.9,), "grid": 64}, {"grid": 64, "probs": [0.9], "scale": 1}),
            "contours": ({"params": ["a", "c"], "bounds": True}, {"bounds": True, "params": [0, 2], "probs": (0.68, 0.95)})}
    for st in posterior.STATS:
        one, two = ({st.key: v, "bounds": b, "marginals": True if st.key != "marginals" else v} for v, b in zip(asks[st.key], ({"a": (0, None)}, [(0.0, np.inf), None, None])))
        r1, r2 = st.resolve(one, names, 3, None), st.resolve(two, names, 3, None)
        assert r1 == r2 and hash(r1) == hash(r2) and st.group(r1) == st.group(r2), st.key
        assert (r1.bounds is not None) == (st.key in ("marginals", "contours")) and st.group(r1)[1] == (r1.bounds is not None)
    assert posterior.MARGINALS.resolve({"marginals": True, "bounds": {"a": (0, None)}}, names, 3, None).bounds == ((0.0, -np.inf, -np.inf), (np.inf, np.inf, np.inf))
    assert posterior.CONTOURS.resolve({"contours": asks["contours"][0], "bounds": {"a": (0, None)}}, names, 3, None).bounds == ((0.0, -np.inf), (np.inf, np.inf))


def _wave():
    """five roots of three parameters: what each asks for, its names, and a measure that records its calls"""
    m1 = {"probs": (0.9,), "grid": 64}
    con = {"params": ["a", "c"], "grid": 32}
    asks = [dict(information=True, summary=(0.68,), marginals=m1, covariance=True),
            dict(summary=(0.9,), marginals=dict(m1), contours=con, covariance=True),
            dict(information=True, marginals={"probs": (0.9,), "grid": 128}, contours=dict(con), covariance=True),
            dict(marginals=m1, bounds={"a": (0, None)}, contours=con, covariance=True),         # (its third parameter is e: the contours do not fit)
            dict(marginals=m1, bounds={"c": (0, 1)}, covariance=True)]                          # (its third parameter is d: the bounds do not fit)
    names = [["a", "b", "c"]] * 3 + [["a", "b", "e"], ["a", "b", "d"]]
    ready = [posterior.Asking(i, posterior.System(1000 + i, 3, 50 + i, 3, 2000 + i, 3000 + i), posterior.values_of(v.get), nm, None)
             for i, (v, nm) in enumerate(zip(asks, names))]
    calls = []

    def measure(st, systems, requests):
        assert len(systems) == len(requests) and len(set(st.group(r) for r in requests)) == 1
        calls.append((st.key, requests[0].bounds is not None, [s.params - 1000 for s in systems]))
        return [(st.key, s.params - 1000) for s in systems]
    return asks, names, ready, calls, measure


def test_the_wave_rule_who_shares_a_call_and_who_fails_alone():
    asks, names, ready, calls, measure = _wave()
    found, failed, still = posterior.measure_wave(ready, measure=measure)
    # one call per statistic, distinct spec and form, the groups in sorted order, the roots in theirs
    assert calls == [("information", False, [0, 2]),
                     ("summary", False, [0]), ("summary", False, [1]),
                     ("marginals", False, [0, 1]), ("marginals", True, [3]), ("marginals", False, [2]),
                     ("contours", False, [1, 2]),
                     ("covariance", False, [0, 1, 2])]
    # the two unfit roots fail alone, in the modules' words, and are in no later call
    with pytest.raises(ValueError) as bounds_err:
        marginals.bounds_spec(asks[4]["bounds"], names=names[4], marginals=asks[4]["marginals"])
    with pytest.raises(ValueError) as params_err:
        contours.spec(asks[3]["contours"], ndim=3, names=names[3])
    assert sorted(failed) == [3, 4] and all(type(e) is ValueError for e in failed.values())
    assert str(failed[4]) == str(bounds_err.value) and "'c' not among the parameters in use (a, b, d)" in str(failed[4])
    assert str(failed[3]) == str(params_err.value) and "the parameter 'c' is not among the names ['a', 'b', 'e']" in str(failed[3])
    assert [a.id for a in still] == [0, 1, 2]
    assert not any(4 in ids for _, _, ids in calls) and not any(3 in ids for key, _, ids in calls if key == "covariance")
    # every other root has a block, and its request, for everything it asked for and for nothing else
    for i in (0, 1, 2):
        assert set(found[i]) == set(asks[i]) - {"bounds"}
        for key, (blk, req) in found[i].items():
            assert blk == (key, i) and req == posterior.BY_KEY[key].resolve(posterior.values_of(asks[i].get), names[i], 3, None)
    assert found[2]["contours"][1].spec[3] == (0, 2) and found[3]["marginals"][1].bounds == ((0.0, -np.inf, -np.inf), (np.inf,) * 3)


def test_the_wave_rule_without_requests_calls_nothing():
    ready = [posterior.Asking(i, posterior.System(1, 3, 50, 3, 2, 3), posterior.values_of({}.get), None, None) for i in range(2)]
    found, failed, still = posterior.measure_wave(ready, measure=lambda *a: pytest.fail("a call without a request"))
    assert found == {0: {}, 1: {}} and failed == {} and still == ready


def test_the_host_route_loops_over_the_table_in_numpy():
    ch = gaussian_chain(seed=11, n=200, d=3, weights="int")
    lo = float(ch[:, 2].min()) - 0.25
    kw = dict(information=True, summary=(0.9,), marginals={"grid": 64}, bounds={"p0": (lo, None)}, contours={"grid": 32, "bounds": True}, covariance=True)
    m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), **kw)
    lnE, info = m.evidence(info=True)
    assert [k for k in info if k in posterior.KEYS] == list(posterior.KEYS)
    samples, lnp, _ = m.gd.arrays("s1")
    a, x, logLmax = m.gd.data["s1"].adjusted_weights, np.asarray(samples, dtype=np.float64)[:, :3], np.amax(lnp)
    fs, names = lnp - logLmax, ["p0", "p1", "p2"]
    bnd = marginals.bounds_spec(kw["bounds"], names=names, marginals=kw["marginals"])
    csp = contours.spec(kw["contours"], ndim=3, names=names)
    cbnd = contours.bounds_spec(kw["contours"], names=names, ndim=3, bounds=kw["bounds"])
    want = {"information": information.build(information.moments(a, fs), logLmax, lnE),
            "summary": summary.build(summary.measure(a, x, fs, summary.targets((0.9,))), (0.9,), logLmax, names),
            "marginals": marginals.build(marginals.measure_bounded(a, x, bnd, *marginals.spec(kw["marginals"])), marginals.spec(kw["marginals"]), names),
            "contours": contours.build(contours.measure_bounded(a, x, csp[3], cbnd, *csp[:3]), csp, names),
            "covariance": covariance.build(covariance.measure(a, x), names)}
    assert info["marginals"]["at_lo"][0] == 1.0 and info["contours"]["at_lo"][0] == 1.0 and info["summary"]["status"] == 0
    for st in posterior.STATS:
        assert _same(info[st.key], want[st.key]), st.key
        assert st.attr is None or getattr(m, st.attr) is info[st.key]
