#!/usr/bin/env python
"""One SHA-256 per (route, request) cell of a fixed matrix of the statistics next to ln E (posterior.py), for comparing two commits bit
for bit: run it in a worktree of each on the same machine and compare the two files.

    python tools/posterior_bits.py [--routes host_numpy,host_library,resident,farm,farm_fallback,tension] [--out FILE.json]

A digest covers every float of the returned ln E and info as raw bytes (ints, strings and keys as text; timings left out) and the lines
the package logged.  The cells of doubly-invalid calls record the exception's type and message.  ``host_numpy`` needs no GPU.
"""
import argparse
import hashlib
import json
import logging
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

_TD = [""]
ROUTES = ("host_numpy", "host_library", "resident", "farm", "farm_fallback", "tension")
M1 = {"probs": (0.9,), "grid": 64}
EVERY = dict(information=True, summary=(0.9,), marginals=M1, contours={"grid": 32}, covariance=True)
REQUESTS = {
    "information": dict(information=True), "summary": dict(summary=True), "marginals": dict(marginals=M1), "contours": dict(contours={"grid": 32, "params": [0, 2]}),
    "covariance": dict(covariance=True), "all": EVERY,
    "bounds_ranges": dict(EVERY, bounds="ranges", contours={"grid": 32, "bounds": True}),
    "bounds_mapping": dict(EVERY, bounds={"p1": (-40.0, None)}),
    "jackknife_information": dict(information=True, jackknife=4),
    "thinned": dict(EVERY, thinlen=2),
}


def feed(h, x):
    """every float as its bytes, everything else as text, dicts by sorted key"""
    if isinstance(x, dict):
        for k in sorted(x):
            if k != "kernel_ms":
                h.update(("{%s}" % k).encode())
                feed(h, x[k])
    elif isinstance(x, (str, bytes, bool, int, type(None))):
        h.update(repr(x).encode())
    elif isinstance(x, (list, tuple)) and any(isinstance(v, (str, dict, list, tuple)) for v in x):
        for v in x:
            feed(h, v)
    else:
        a = np.asarray(x)
        h.update(("[%s%s]" % (a.dtype.kind, a.shape)).encode())
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes() if a.dtype.kind in "fiub" else repr(a.tolist()).encode())


class Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def cell(call):
    """the digest of what ``call()`` returns and logs, or the exception it raises"""
    log, logger = Lines(), logging.getLogger("mcevidence_amd")
    logger.addHandler(log)
    try:
        out = call()
    except Exception as e:
        return {"raises": type(e).__name__, "message": str(e)}
    finally:
        logger.removeHandler(log)
    h = hashlib.sha256()
    feed(h, out)
    feed(h, [ln.replace(_TD[0], "<td>") for ln in log.lines])      # (the temporary directory differs between runs)
    return {"sha256": h.hexdigest(), "lines": len(log.lines)}


def write_roots(td):
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    roots = []
    for r in range(3):
        chains = [gaussian_chain(seed=700 + 2 * r + c, n=300, d=3, weights="int", cov="corr") for c in range(2)]
        lo = min(float(ch[:, 2].min()) for ch in chains) - 0.5
        roots.append(os.path.join(td, "bits%d" % r))
        write_cosmomc_chains(roots[-1], chains, [("p0", lo, None), ("p1", -50.0, 50.0), ("p2", -50.0, None)], fmt="%.17g")
    return roots


def run_route(route, roots, kw):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm, tension
    if route in ("host_numpy", "host_library"):
        from helpers import OracleBackend
        kw = dict(kw)
        jack = kw.pop("jackknife", None)
        back = {"backend": OracleBackend()} if route == "host_numpy" else {}
        if jack is not None and route == "host_numpy":
            return "skipped: the jackknife's search runs on the device"
        m = pkg.MCEvidence(roots[0], kmax=3, verbose=1, jackknife=jack, **back, **kw)
        return m.evidence(info=True)
    if route == "resident":
        return pkg.evidence_from_files(roots[0], kmax=3, info=True, verbose=1, require_resident=True, **kw)
    if route == "farm":
        return farm.evidence_many_from_files(roots, kmax=3, info=True, **kw)
    if route == "farm_fallback":
        return farm.evidence_many_from_files(roots, kmax=3, info=True, thin_corr=[None, True, None], **{k: v for k, v in kw.items() if k != "thinlen"})
    kw = {k: v for k, v in kw.items() if k not in ("information", "covariance")}
    return tension.evidence_tension(roots[0], roots[1], roots[2], shared=3, kmax=3, **kw)


def invalid_calls(roots, device):
    from mcevidence_amd import farm, resident
    from mcevidence_amd.evidence import MCEvidence
    calls = {"plan_summary_marginals": lambda: resident.plan(summary="x", marginals="y"),
             "plan_marginals_bounds": lambda: resident.plan(marginals="y", bounds="z"),
             "plan_bounds_contours": lambda: resident.plan(marginals=True, bounds="z", contours={"zz": 1}),
             "plan_contours_covariance": lambda: resident.plan(contours={"zz": 1}, covariance=3),
             "host_information_summary": lambda: MCEvidence(roots[0], verbose=0, nbatch=2, brange=[1, 2], information=True, summary="x")}
    if device:
        calls.update({"farm_marginals_bounds": lambda: farm.evidence_many_from_files(roots, marginals=[None, {"zz": 1}, None], bounds=["z", None, None]),
                      "farm_bounds_contours": lambda: farm.evidence_many_from_files(roots, marginals=True, bounds=[None, None, "z"], contours=[{"zz": 1}, None, None]),
                      "farm_contours_covariance": lambda: farm.evidence_many_from_files(roots, contours=[None, {"zz": 1}, None], covariance=[3, None, None]),
                      "resident_files_marginals_covariance": lambda: resident.evidence_from_files(roots[0], marginals="y", covariance=3)})
    return {name: cell(fn) for name, fn in calls.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posterior_stats", "bits.json"))
    args = ap.parse_args(argv)
    routes = [r for r in args.routes.split(",") if r]
    logging.basicConfig(level=logging.WARNING)
    doc = {"cells": {}, "invalid": {}}
    with tempfile.TemporaryDirectory() as td:
        _TD[0] = td
        roots = write_roots(td)
        for route in routes:
            for name, kw in REQUESTS.items():
                np.random.seed(0)
                got = cell(lambda: run_route(route, roots, kw))
                # (temporary paths differ between runs: a message is kept without them)
                if "message" in got:
                    got["message"] = got["message"].replace(td, "<td>")
                doc["cells"]["%s/%s" % (route, name)] = got
        doc["invalid"] = invalid_calls(roots, device=any(r != "host_numpy" for r in routes))
        for got in doc["invalid"].values():
            if "message" in got:
                got["message"] = got["message"].replace(td, "<td>")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d cells, %d invalid calls -> %s" % (len(doc["cells"]), len(doc["invalid"]), args.out))
    return doc


if __name__ == "__main__":
    main()
