"""Command line: ``python MCEvidence.py <root> [flags]`` -- same flags as the reference
CLI (``/root/reference/MCEvidence.py:1342-1473``)."""
from __future__ import annotations

import logging
import sys
from argparse import ArgumentParser

from . import prior
from .evidence import MCEvidence

desc = "Planck Chains MCEvidence. Returns the log Bayesian Evidence computed using the kth NN"
cite = """
**
When using this code in published work, please cite the following paper: **
Heavens et. al. (2017)
Marginal Likelihoods from Monte Carlo Markov Chains
https://arxiv.org/abs/1704.03472
"""


def build_parser(prog=None):
    p = ArgumentParser(prog=prog, add_help=True, description=desc, epilog=cite)
    p.add_argument("root_name", help="Root filename for MCMC chains")
    p.add_argument("-k", "--kmax", dest="kmax", default=2, type=int, help="maximum k of the k-th nearest neighbour")
    p.add_argument("-ic", "--idchain", dest="idchain", default=0, type=int,
                   help="Which chain to use - e.g. 1 means read only *_1.txt (default: all available)")
    p.add_argument("-np", "--ndim", dest="ndim", default=None, type=int, help="How many parameters to use (default: all)")
    p.add_argument("--paramsfile", dest="paramsfile", default="", type=str,
                   help="text file with additional parameter names to consider cosmological")
    p.add_argument("--burn", "--burnlen", dest="burnlen", default=0, type=float,
                   help="Burn-in length or fraction; burnlen<1 is a fraction, e.g. 0.3 = 30%%")
    p.add_argument("--thin", "--thinlen", dest="thinlen", default=0, type=float,
                   help="Thinning: 0<thinlen<1 Poisson-resampled weights; thinlen>1 weighted thinning")
    p.add_argument("--thin-corr", dest="thin_corr", nargs="?", const=True, default=None, type=float, metavar="SCALE",
                   help="thin by SCALE (default 1) times the measured autocorrelation length of the chains instead of a given --thin; "
                        "write it after root_name, or as --thin-corr=SCALE: directly in front of root_name it would take the root for SCALE")
    p.add_argument("--converge", dest="converge", nargs="?", const=True, default=None, type=float, metavar="THRESHOLD",
                   help="measure the Gelman-Rubin R-1 of the burned chains and print it before the ln(B) lines; with THRESHOLD, warn when R-1 "
                        "exceeds it.  Write it after root_name, or as --converge=THRESHOLD")
    p.add_argument("--converge-by", dest="converge_by", default="auto", choices=("auto", "chains", "halves"),
                   help="the segments R-1 compares: whole chains, halves of every chain, or (auto) chains when there are at least two")
    p.add_argument("-vb", "--verbose", dest="verbose", default=1, type=int, help="0: WARNINGS, 1: INFO, 2: DEBUG")
    p.add_argument("-pv", "--pvolume", dest="priorvolume", default=None, type=float,
                   help="prior volume to use; if *.ranges exists the volume estimated from it is used")
    p.add_argument("--allparams", action="store_true", help="use all parameters, not only the cosmological ones")
    p.add_argument("--cross", action="store_true",
                   help="split the chain(s) in two and estimate the cross evidence (otherwise auto evidence)")
    p.add_argument("--resident", action="store_true",
                   help="keep the chain on the GPU from the text files to ln E (mcevidence_amd.resident); falls back to the host route where it does not apply")
    p.add_argument("--farm", action="store_true",
                   help="root_name is a text file with one chain root per line ('#' starts a comment): all roots in batched GPU passes "
                        "(mcevidence_amd.farm); a root the farm does not cover takes the per-root route")
    p.add_argument("--device-eig", dest="device_eig", action="store_true",
                   help="solve the covariance eigen-systems of the device feeders on the GPU (HipBackend(device_eig=True)) instead of on the host")
    p.add_argument("--jackknife", dest="jackknife", nargs="?", const=16, default=None, type=int, metavar="G",
                   help="delete-a-group jackknife error bars on ln(B) from one neighbour search, G groups (default 16); prints ln(B)[k] = x +- sigma "
                        "(conservative, not a calibrated 1 sigma); write it after root_name, or as --jackknife=G")
    p.add_argument("--jackknife-by", dest="jackknife_by", choices=("blocks", "chains"), default="blocks",
                   help="the groups: contiguous blocks of the burned / thinned chain, or one group per chain file")
    p.add_argument("--information", dest="information", action="store_true",
                   help="print <ln L>, the Bayesian model dimensionality d, N_eff and D_KL[k] = <ln L> - ln(B)[k] before the ln(B) lines "
                        "(with --jackknife: each with +- sigma); D_KL is relative to the flat prior over the given volume")
    p.add_argument("--summary", dest="summary", nargs="*", default=None, type=float, metavar="P",
                   help="print the weighted mean, standard deviation, equal-tailed limits (probabilities P ...; default 0.68 0.95) and the "
                        "best-fit sample of every parameter used, after the information lines and before the ln(B) lines: logged with them "
                        "at -vb 1, printed where the ln(B) lines are printed (--farm, --jackknife) at -vb 0; write it after root_name")
    p.add_argument("--marginals", dest="marginals", nargs="*", default=None, type=float, metavar="P",
                   help="print the mode, the highest-posterior-density limits with their number of pieces (probabilities P ...; default 0.68 "
                        "0.95) and the bandwidth h of the 1-D marginal density of every parameter used, after the summary lines and before "
                        "the ln(B) lines; write it after root_name")
    p.add_argument("--marginals-grid", dest="marginals_grid", default=None, type=int, metavar="G", choices=(64, 128, 256, 512, 1024),
                   help="with --marginals: the grid points of a density (default 512)")
    p.add_argument("--marginals-scale", dest="marginals_scale", default=None, type=float, metavar="S",
                   help="with --marginals: the bandwidth as a multiple of the normal-reference rule (default 1)")
    p.add_argument("--marginals-out", dest="marginals_out", default=None, metavar="FILE.npz",
                   help="with --marginals: write the names, the grid points and the densities of every parameter to FILE.npz, one set per root")
    p.add_argument("--bounds", dest="bounds", nargs="*", default=None, metavar="NAME=LO:HI",
                   help="with --marginals: honour hard prior bounds in the 1-D densities (a linear boundary kernel; the grid ends on the bound). "
                        "Without a value: the bounds of the root's .ranges or log.param file; or NAME=LO:HI ..., an empty side or N: open")
    p.add_argument("--contours", dest="contours", nargs="*", default=None, type=float, metavar="P",
                   help="also report the 2-D joint posterior density of every pair of the chosen parameters: its mode and, per probability P "
                        "(default 0.68 0.95), the contour level and the number of grid cells it encloses")
    p.add_argument("--contours-params", dest="contours_params", nargs="+", default=None, metavar="NAME",
                   help="with --contours: the parameters (names or column indices, 2 to 32; default: all of the parameters used, at most 32)")
    p.add_argument("--contours-grid", dest="contours_grid", default=None, type=int, metavar="G", choices=(32, 64),
                   help="with --contours: the grid points per axis (default 64)")
    p.add_argument("--contours-scale", dest="contours_scale", default=None, type=float, metavar="S",
                   help="with --contours: the bandwidth as a multiple of the normal-reference rule (default 1)")
    p.add_argument("--contours-bounds", dest="contours_bounds", nargs="*", default=None, metavar="NAME=LO:HI",
                   help="with --contours: honour hard prior bounds in the 2-D densities (the linear boundary kernel of the product kernel; the grids end on "
                        "the bounds). Without a value: the bounds of the root's .ranges or log.param file; or NAME=LO:HI ..., an empty side or N: open")
    p.add_argument("--contours-out", dest="contours_out", default=None, metavar="FILE.npz",
                   help="with --contours: write the names, the pairs, the two grid axes, the densities and the levels of every pair to FILE.npz, one set per root")
    p.add_argument("--tension", dest="tension", nargs=2, default=None, metavar=("ROOT_A", "ROOT_B"),
                   help="tension between the data sets of the roots ROOT_A and ROOT_B under one model, root_name being their JOINT run: the three "
                        "roots in one batched GPU pass (mcevidence_amd.tension), then ln R, ln I, the suspiciousness ln S, the dimensionality d "
                        "with its p-value, and the Gaussian parameter shift in the parameters A and B share; composes with --jackknife, --burn, "
                        "--thin, --thin-corr, -k, --cross, --converge and --summary (all three roots take them), not with --farm or --resident; write it "
                        "after root_name")
    p.add_argument("--shift-kde", dest="shift_kde", nargs="?", const=1, default=None, type=int, metavar="BOOST",
                   help="with --tension: the non-Gaussian parameter shift too -- the posterior mass of the parameter difference above the density "
                        "at no difference, by a leave-one-out kernel density estimate on the difference chain (mcevidence_amd.shift_kde); BOOST "
                        "(default 1) pairs every row of A with that many rows of B; one more line after the Gaussian shift: p [p_lo, p_hi], "
                        "sigma, n_local, rows and the bandwidth h")
    p.add_argument("--shift-bandwidth", dest="shift_bandwidth", default=None, type=float, metavar="SCALE",
                   help="with --shift-kde: the bandwidth as a multiple of Silverman's rule (default 1; raise it where n_local is small)")
    p.add_argument("--gain-knn", dest="gain_knn", nargs="?", const=4, default=None, type=int, metavar="K",
                   help="with --tension: the information gain too -- the relative entropy D_KL(AB || A), D_KL(AB || B), D_KL(A || B) and "
                        "D_KL(B || A) between the runs' posteriors from nearest-neighbour distances (mcevidence_amd.divergence), for the ranks "
                        "k = 1 .. K (default 4, at most 16), each with a delete-a-block jackknife error bar; four more lines after the shift")
    p.add_argument("--gain-groups", dest="gain_groups", default=None, type=int, metavar="G",
                   help="with --gain-knn or --divergence: the jackknife blocks of each chain (default 8; 0: no error bar; at most 64)")
    p.add_argument("--divergence", dest="divergence", nargs="+", default=None, metavar=("ROOT_Q", "K"),
                   help="print the relative entropy D_KL(root_name || ROOT_Q)[k] = x +- sigma, k = 1 .. K (default 4), between the posteriors of the "
                        "two roots over the parameters they share (by name where both have a .paramnames file, else the leading columns), from "
                        "nearest-neighbour distances; composes with --burn, --thin, --thin-corr and -np (both roots take them); write it after "
                        "root_name")
    return p


def _summary_kw(args):
    """--summary, where it was given: True, or the probabilities"""
    if args.summary is None:
        return {}
    return {"summary": tuple(args.summary) if args.summary else True}


def _bounds_kw(args, dest="bounds"):
    """--bounds (``dest="contours_bounds"``: --contours-bounds), where it was given: "ranges", or the mapping of its NAME=LO:HI values"""
    given = getattr(args, dest, None)
    if given is None:
        return {}
    if not given:
        return {"bounds": "ranges"}
    out = {}
    for item in given:
        name, eq, pair = item.partition("=")
        lo, colon, hi = pair.partition(":")
        if not name or not eq or not colon:
            raise ValueError("bounds=%r: NAME=LO:HI expected" % (item,))
        out[name] = tuple(None if v.strip() in ("", "N", "None") else v.strip() for v in (lo, hi))
    return {"bounds": out}


def _marginals_kw(args):
    """--marginals / --marginals-grid / --marginals-scale, where the first was given, and --bounds with them"""
    if args.marginals is None:
        return {}
    if args.marginals_grid is None and args.marginals_scale is None:
        return dict({"marginals": tuple(args.marginals) if args.marginals else True}, **_bounds_kw(args))
    kw = {"probs": tuple(args.marginals) if args.marginals else True}
    if args.marginals_grid is not None:
        kw["grid"] = args.marginals_grid
    if args.marginals_scale is not None:
        kw["scale"] = args.marginals_scale
    return dict({"marginals": kw}, **_bounds_kw(args))


def _contours_kw(args):
    """--contours / --contours-params / --contours-grid / --contours-scale / --contours-bounds, where the first was given"""
    if args.contours is None:
        return {}
    bounds = _bounds_kw(args, "contours_bounds")
    if args.contours_params is None and args.contours_grid is None and args.contours_scale is None and not bounds:
        return {"contours": tuple(args.contours) if args.contours else True}
    kw = dict({"probs": tuple(args.contours) if args.contours else True}, **bounds)
    if args.contours_params is not None:
        kw["params"] = [int(v) if v.isdigit() else v for v in args.contours_params]
    if args.contours_grid is not None:
        kw["grid"] = args.contours_grid
    if args.contours_scale is not None:
        kw["scale"] = args.contours_scale
    return {"contours": kw}


def _print_stats(info, logged=False, information=True):
    """the lines of the statistics (posterior.STATS' order: information, summary, marginals, contours), before the ln(B) lines; ``logged``: the
    route has logged those after the information lines already; ``information=False``: without the information lines"""
    from .posterior import STATS
    for st in STATS:
        if (info or {}).get(st.key) and (information if st.key == "information" else not logged):
            for line in st.lines(info[st.key]):
                print(line)


def _save_stats(args, roots, infos):
    """--marginals-out and --contours-out, where they were given"""
    from . import contours, marginals
    for path, module in ((args.marginals_out, marginals), (args.contours_out, contours)):
        if path is not None:
            module.save(path, roots, infos)


def _information_kw(args):
    """--information, where it was given"""
    return {"information": True} if args.information else {}


def _jackknife_kw(args):
    """--jackknife / --jackknife-by, where the first was given (the resident route and the farm take them as a keyword)"""
    return {} if args.jackknife is None else {"jackknife": {"groups": args.jackknife, "by": args.jackknife_by}}


def _print_lnb(mle, info):
    """the ln(B) lines: with a jackknife, x +- sigma as the host route prints them; returns whether it did"""
    jk = (info or {}).get("jackknife")
    if jk is None:
        for k in range(1, len(mle) + 1):
            print("   ln(B)[k={}] = {}".format(k, mle[k - 1]))
        return False
    for k in range(1, len(jk["lnE"]) + 1):
        print("   ln(B)[k={}] = {} \u00b1 {}".format(k, jk["lnE"][k - 1], jk["sigma"][k - 1]))
    return jk


def _print_jackknife_note(jk):
    print("* \u00b1: delete-a-group jackknife over {} {} (conservative, not a calibrated 1 sigma).".format(jk["groups"], jk["by"]))


def _backend_kw(args):
    """the backend the flags ask for; nothing when they ask for none (the default backend, as ever)"""
    if not args.device_eig:
        return {}
    from .evidence import HipBackend
    return {"backend": HipBackend(device_eig=True)}


def _thin_kw(args):
    """--thin-corr, where it was given"""
    return {} if args.thin_corr is None else {"thin_corr": args.thin_corr}


def _converge_kw(args):
    """--converge / --converge-by, where the first was given"""
    return {} if args.converge is None else {"converge": args.converge, "converge_by": args.converge_by}


def _print_converge(info):
    """the R-1 line, before the ln(B) lines"""
    from .chains import conv_line
    if (info or {}).get("converge"):
        print(conv_line(info["converge"]))


def farm_main(args):
    """``--farm``: every root of the list file, each with the ndim and the prior volume a single run would compute for it"""
    import copy
    from .farm import evidence_many_from_files
    with open(args.root_name) as fh:
        roots = [ln.split("#", 1)[0].strip() for ln in fh]
    roots = [r for r in roots if r]
    pvols, ndims = [], []
    for r in roots:
        a = copy.copy(args)
        a.root_name = r
        pvols.append(prior.get_prior_volume(a, cosmo=not args.allparams))      # (sets a.ndim, as for one root)
        ndims.append(a.ndim)
    logging.getLogger("mcevidence_amd").setLevel(
        logging.DEBUG if args.verbose > 1 else (logging.INFO if args.verbose == 1 else logging.WARNING))
    want_info = args.converge is not None or args.information or args.jackknife is not None or args.summary is not None or args.marginals is not None or \
        args.contours is not None
    outs = evidence_many_from_files(roots, kmax=args.kmax, ndim=ndims, priorvolume=pvols, burnlen=args.burnlen, thinlen=args.thinlen,
                                    idchain=args.idchain, split=args.cross, info=want_info, **_thin_kw(args), **_converge_kw(args),
                                    **_information_kw(args), **_summary_kw(args), **_marginals_kw(args), **_contours_kw(args), **_jackknife_kw(args),
                                    **_backend_kw(args))
    infos = [o[1] for o in outs] if want_info else [None] * len(outs)
    outs = [o[0] for o in outs] if want_info else outs
    note = None
    for r, mle, inf in zip(roots, outs, infos):
        print()
        print("Using file: ", r)
        _print_converge(inf)
        _print_stats(inf)
        note = _print_lnb(mle, inf) or note
    _save_stats(args, roots, infos)
    if note:
        _print_jackknife_note(note)
    print("* ln(B)[k] is the natural logarithm of the Baysian evidence estimated using the kth Nearest Neighbour.")
    print("")
    return outs


def _shift_kw(args):
    """--shift-kde / --shift-bandwidth, where the first was given"""
    if args.shift_kde is None:
        return {}
    return {"shift": "both", "boost": args.shift_kde, "bandwidth_scale": 1.0 if args.shift_bandwidth is None else args.shift_bandwidth}


def _gain_kw(args):
    """--gain-knn / --gain-groups, where the first was given"""
    if args.gain_knn is None:
        return {}
    return {"gain": "knn", "gain_k": args.gain_knn, "gain_groups": 8 if args.gain_groups is None else args.gain_groups}


def divergence_main(args):
    """``--divergence ROOT_Q [K]``: D_KL(root_name || ROOT_Q)[k] over the shared parameters, from the host rows of two ``MCEvidence``
    objects; both roots take --burn, --thin, --thin-corr and -np"""
    import copy
    from . import divergence, tension
    from .summary import param_names
    roots = [args.root_name, args.divergence[0]]
    K = int(args.divergence[1]) if len(args.divergence) > 1 else 4
    logging.getLogger("mcevidence_amd").setLevel(
        logging.DEBUG if args.verbose > 1 else (logging.INFO if args.verbose == 1 else logging.WARNING))
    data, names = [], []
    for r in roots:
        a = copy.copy(args)
        a.root_name = r
        pvol = prior.get_prior_volume(a, cosmo=not args.allparams)      # (sets a.ndim, as for one root)
        m = MCEvidence(r, ndim=a.ndim, priorvolume=pvol, idchain=args.idchain, kmax=args.kmax, verbose=0, burnlen=args.burnlen, thinlen=args.thinlen,
                       **_thin_kw(args), **_backend_kw(args))
        data.append(tension._host_rows(m))
        names.append(param_names(r, m.ndim))
    shared, ip, iq = tension._pair_shared(names[0], names[1])
    (xp, wp), (xq, wq) = data
    out = tension.knn_divergence(xp[:, ip], wp, xq[:, iq], wq, kmax=K, groups=8 if args.gain_groups is None else args.gain_groups, names=shared)
    print()
    print("Relative entropy of {} against {}".format(*roots))
    for line in divergence.lines(out, label="D_KL({} ‖ {})".format(*roots)):
        print(line)
    print(tension.FOOTNOTE_GAIN)
    print("")
    return out


def tension_main(args):
    """``--tension ROOT_A ROOT_B``: the three roots as ``--farm`` prints roots, then the tension lines and their footnote.  ``--cross``,
    ``--converge``, ``--summary`` and ``--marginals`` go to all three roots (``--information`` is always set); ``--farm`` and ``--resident`` name another
    route for ``root_name`` and are refused"""
    import copy
    from . import tension
    roots = [args.tension[0], args.tension[1], args.root_name]
    pvols, ndims = [], []
    for r in roots:
        a = copy.copy(args)
        a.root_name = r
        pvols.append(prior.get_prior_volume(a, cosmo=not args.allparams))      # (sets a.ndim, as for one root)
        ndims.append(a.ndim)
    logging.getLogger("mcevidence_amd").setLevel(
        logging.DEBUG if args.verbose > 1 else (logging.INFO if args.verbose == 1 else logging.WARNING))
    ea, eb, eab, info = tension.evidence_tension(roots[0], roots[1], roots[2], kmax=args.kmax, ndim=ndims, priorvolume=pvols, burnlen=args.burnlen,
                                                 thinlen=args.thinlen, idchain=args.idchain, split=args.cross, **_thin_kw(args), **_converge_kw(args),
                                                 **_summary_kw(args), **_marginals_kw(args), **_contours_kw(args), **_jackknife_kw(args), **_backend_kw(args),
                                                 **_shift_kw(args), **_gain_kw(args))
    note = None
    for r, mle, inf in zip(roots, (ea, eb, eab), info["roots"]):
        print()
        print("Using file: ", r)
        _print_converge(inf)
        _print_stats(inf)
        note = _print_lnb(mle, inf) or note
    _save_stats(args, roots, info["roots"])
    print()
    print("Tension of {} and {} (joint run: {})".format(*roots))
    for line in tension.lines(info["tension"]):
        print(line)
    if note:
        _print_jackknife_note(note)
    print("* ln(B)[k] is the natural logarithm of the Baysian evidence estimated using the kth Nearest Neighbour.")
    print(tension.FOOTNOTE)
    if args.shift_kde is not None:
        print(tension.FOOTNOTE_KDE)
    if args.gain_knn is not None:
        print(tension.FOOTNOTE_GAIN)
    print("")
    return ea, eb, eab, info


def main(argv=None):
    args = build_parser(prog="MCEvidence.py").parse_args(argv)
    if args.paramsfile:
        with open(args.paramsfile) as fh:
            new = [ln.strip() for ln in fh if ln.strip() and "#" not in ln]
        print("adding the following names to the cosmological parameter list:", new)
        for n in new:
            if n not in prior.cosmo_params_list:
                prior.cosmo_params_list.append(n)
    if (args.shift_kde is not None or args.shift_bandwidth is not None) and args.tension is None:
        build_parser(prog="MCEvidence.py").error("--shift-kde and --shift-bandwidth belong to --tension ROOT_A ROOT_B")
    if args.shift_bandwidth is not None and args.shift_kde is None:
        build_parser(prog="MCEvidence.py").error("--shift-bandwidth belongs to --shift-kde")
    if args.shift_kde is not None and args.shift_kde < 1:
        build_parser(prog="MCEvidence.py").error("--shift-kde BOOST: a positive number of offsets expected")
    if args.shift_bandwidth is not None and not args.shift_bandwidth > 0.0:
        build_parser(prog="MCEvidence.py").error("--shift-bandwidth SCALE: a positive number expected")
    if args.gain_knn is not None and args.tension is None:
        build_parser(prog="MCEvidence.py").error("--gain-knn belongs to --tension ROOT_A ROOT_B")
    if args.gain_groups is not None and args.gain_knn is None and args.divergence is None:
        build_parser(prog="MCEvidence.py").error("--gain-groups belongs to --gain-knn or --divergence")
    if args.gain_knn is not None and not 1 <= args.gain_knn <= 16:
        build_parser(prog="MCEvidence.py").error("--gain-knn K: 1 .. 16 expected")
    if args.gain_groups is not None and args.gain_groups != 0 and not 2 <= args.gain_groups <= 64:
        build_parser(prog="MCEvidence.py").error("--gain-groups G: 0, or 2 .. 64 expected")
    if args.divergence is not None:
        if len(args.divergence) > 2 or (len(args.divergence) == 2 and not (args.divergence[1].isdigit() and 1 <= int(args.divergence[1]) <= 16)):
            build_parser(prog="MCEvidence.py").error("--divergence ROOT_Q [K]: one root and, optionally, K in 1 .. 16 expected")
        if args.tension is not None or args.farm or args.resident:
            build_parser(prog="MCEvidence.py").error("--divergence compares root_name with ROOT_Q: it does not combine with --tension, --farm or --resident")
        return divergence_main(args)
    if (args.marginals_grid is not None or args.marginals_scale is not None or args.marginals_out is not None) and args.marginals is None:
        build_parser(prog="MCEvidence.py").error("--marginals-grid, --marginals-scale and --marginals-out belong to --marginals")
    if args.bounds is not None and args.marginals is None:
        build_parser(prog="MCEvidence.py").error("--bounds belongs to --marginals")
    if (args.contours_params is not None or args.contours_grid is not None or args.contours_scale is not None or args.contours_out is not None or
            args.contours_bounds is not None) and args.contours is None:
        build_parser(prog="MCEvidence.py").error("--contours-params, --contours-grid, --contours-scale, --contours-bounds and --contours-out belong to --contours")
    if args.tension is not None:
        if args.farm or args.resident:
            build_parser(prog="MCEvidence.py").error("--tension runs its three roots in one batched pass: it does not combine with --farm or --resident")
        return tension_main(args)
    if args.farm:
        return farm_main(args)
    prior_volume = prior.get_prior_volume(args, cosmo=not args.allparams)
    logging.getLogger("mcevidence_amd").setLevel(
        logging.DEBUG if args.verbose > 1 else (logging.INFO if args.verbose == 1 else logging.WARNING))
    print()
    print("Using file: ", args.root_name)
    if args.resident:
        from .resident import evidence_from_files
        want_info = args.jackknife is not None or args.marginals_out is not None or args.contours_out is not None
        out = evidence_from_files(args.root_name, split=args.cross, ndim=args.ndim, priorvolume=prior_volume, idchain=args.idchain,
                                  kmax=args.kmax, verbose=args.verbose, burnlen=args.burnlen, thinlen=args.thinlen, info=want_info,
                                  **_thin_kw(args), **_converge_kw(args), **_information_kw(args), **_summary_kw(args), **_marginals_kw(args), **_contours_kw(args),
                                  **_jackknife_kw(args), **_backend_kw(args))
        if want_info:
            out, inf = out
            _save_stats(args, [args.root_name], [inf])
        if args.jackknife is not None:
            _print_stats(inf, logged=args.verbose >= 1, information=False)
            jk = _print_lnb(out, inf)
            if jk:
                _print_jackknife_note(jk)
        print("* ln(B)[k] is the natural logarithm of the Baysian evidence estimated using the kth Nearest Neighbour.")
        print("")
        return out
    mce = MCEvidence(args.root_name, split=args.cross, ndim=args.ndim, priorvolume=prior_volume,
                     idchain=args.idchain, kmax=args.kmax, verbose=args.verbose, burnlen=args.burnlen,
                     thinlen=args.thinlen, **_thin_kw(args), **_converge_kw(args), **_information_kw(args), **_summary_kw(args), **_marginals_kw(args), **_contours_kw(args),
                     **_backend_kw(args))
    _print_converge(getattr(mce, "info", None))
    if args.jackknife is not None:
        mce.jackknife = {"groups": args.jackknife, "by": args.jackknife_by}
        out = mce.evidence()
        jk = mce.info["jackknife"]
        _print_stats(mce.info, logged=args.verbose >= 1)
        for k in range(1, len(jk["lnE"]) + 1):
            print("   ln(B)[k={}] = {} \u00b1 {}".format(k, jk["lnE"][k - 1], jk["sigma"][k - 1]))
        print("* \u00b1: delete-a-group jackknife over {} {} (conservative, not a calibrated 1 sigma).".format(jk["groups"], jk["by"]))
    else:
        out = mce.evidence()
    _save_stats(args, [args.root_name], [getattr(mce, "info", None)])
    print("* ln(B)[k] is the natural logarithm of the Baysian evidence estimated using the kth Nearest Neighbour.")
    print("")
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
