"""Which entry point a whole record folds through: the Python counterpart of the host file's mfe_route / pf_route.

Up to SF_MAX_W nt a sequence is a window and folds on the window kernels.  Past that the library has seven whole-record entry
points: full tables (fold_long, pf_long; up to SF_MAX_LONG), banded tables under the resident base-pair span (fold_banded,
pf_banded; up to SF_MAX_BANDED), and their batches.  mfe_route and pf_route choose among them ("Routes of the
whole-record folds"; tests/test_whole_routes.py pins the table); fold, fold_rows, pf and pf_rows run what they chose; pf_probs
runs the banded partition function with its base-pair probabilities brought out (pf_banded_probs: pf_banded's route, no
route of its own), and pf_mea adds the maximum-expected-accuracy structure of that list (pf_banded_mea, likewise).  No other module of the package calls one of them on an engine.

A caller states its banded policy:
  AUTO    the RNA facade's rule: banded tables when the record is past SF_MAX_LONG, or when a span is resident, the record is
          at least four spans long and the library has the entry point; else full tables.
  ALWAYS  the caller's flag asks for banded tables (--global_span, --global_zscore_span, --global_ensemble_banded), at any
          length.
  NEVER   full tables whatever span is resident (functions.energies, functions.rna_refold, --global_ensemble).
"""
import collections

from . import _lib

AUTO, ALWAYS, NEVER = "auto", "always", "never"
WINDOW = "window"
ENTRY_POINTS = ("fold_long", "fold_long_batch", "fold_banded", "fold_banded_batch", "pf_long", "pf_long_batch", "pf_banded")

# call: WINDOW or the name of an Engine method; limit: the longest record that call takes
Route = collections.namedtuple("Route", "call limit")


def exports(eng):
    """the whole-record entry points the engine's library has, as names of Engine methods"""
    return frozenset(name for name in ENTRY_POINTS if getattr(eng, "has_" + name)())


def mfe_route(L, span=0, many=False, banded=AUTO, exported=ENTRY_POINTS, shape=False, library="?"):
    """The MFE fold of a record of L nt under the resident span, alone or as one row of many (the batch entry points).
    shape: the caller has SHAPE pseudo-energies.  exported / library: exports() of the engine and its library's name."""
    tail = "_batch" if many else ""
    if banded == ALWAYS:
        return Route("fold_banded" + tail, _lib.SF_MAX_BANDED)
    if L <= _lib.SF_MAX_W:
        return Route(WINDOW, _lib.SF_MAX_W)
    if shape:
        raise NotImplementedError("SHAPE soft constraints on a sequence longer than %d nt: the whole-record fold "
                                  "(sf_fold_long) has no pseudo-energy term" % _lib.SF_MAX_W)
    if banded == AUTO:
        if L > _lib.SF_MAX_LONG and span < 1:
            raise ValueError("a sequence of %d nt folds only under md.max_bp_span (sf_fold_banded): without a span "
                             "whole-record folds stop at %d nt" % (L, _lib.SF_MAX_LONG))
        # under a span the band holds the whole fold: the same bytes from 12 L span bytes of tables (sf_fold_banded)
        if L > _lib.SF_MAX_LONG or (span > 0 and 4 * span <= L and "fold_banded" + tail in exported):
            return Route("fold_banded" + tail, _lib.SF_MAX_BANDED)
    if many and "fold_long_batch" not in exported:
        raise _lib.ScanFoldHipError("energies: a sequence of more than %d nt needs sf_fold_long_batch, which this library "
                                    "(%s) does not export" % (_lib.SF_MAX_W, library))
    return Route("fold_long" + tail, _lib.SF_MAX_LONG)


def pf_route(L, span=0, many=False, banded=AUTO, exported=ENTRY_POINTS):
    """The partition function of a record of L nt under the resident span, alone or as one row of many.  There is no banded
    batch: the rows of an ALWAYS caller go through pf_banded one by one, as do those of pf_long without sf_pf_long_batch."""
    if banded == ALWAYS:
        if span < 1:
            raise ValueError("the banded ensemble needs a base-pair span")
        return Route("pf_banded", _lib.SF_MAX_BANDED)
    if L <= _lib.SF_MAX_W:
        return Route(WINDOW, _lib.SF_MAX_W)
    if banded == AUTO:
        raise NotImplementedError("no partition function (and so no centroid / mean base-pair distance) through this "
                                  "facade for a sequence longer than %d nt: only the MFE of a whole record is routed "
                                  "(sf_fold_long); call Engine.pf_long or functions.rna_refold" % _lib.SF_MAX_W)
    return Route("pf_long_batch" if many and "pf_long_batch" in exported else "pf_long", _lib.SF_MAX_LONG)


def _routed(route_fn, eng, L, many, banded, **kw):
    return route_fn(L, eng.max_bp_span, many, banded, exports(eng), **kw).call


def fold(eng, seq, cons=None, banded=AUTO, sc=None):
    """One record -> (mfe_dcal, dot-bracket).  cons: a dot-bracket hard constraint or None; sc: int32 pseudo-energies per
    nucleotide or None (windows only)."""
    if cons is not None and len(cons) != len(seq):
        raise ValueError("constraint string and sequence differ in length")
    call = _routed(mfe_route, eng, len(seq), False, banded, shape=sc is not None)
    if call != WINDOW:
        return getattr(eng, call)(seq, cons)
    if cons is None and sc is None:
        e, db = eng.mfe_trace_batch([seq])
        return e[0], db[0]
    r = eng.fold_constrained([seq], None if cons is None else [cons], None if sc is None else sc[None, :], pf=False)
    return r["mfe"][0], r["structure"][0]


def fold_rows(eng, seqs, banded=NEVER):
    """Many records of any mix of lengths -> their MFEs in dcal/mol, order kept: the whole records in ONE call of their
    batch entry point, then the windows in one mfe_batch per distinct length; an empty row is 0."""
    exported, library = exports(eng), getattr(eng.lib, "_name", "?")
    groups = {}
    for k, s in enumerate(seqs):
        call = mfe_route(len(s), eng.max_bp_span, True, banded, exported, library=library).call
        groups.setdefault((call, len(s)) if call == WINDOW else (call, None), []).append(k)
    out = [0] * len(seqs)
    for whole_records in (True, False):
        for (call, n), ks in groups.items():
            if (call != WINDOW) == whole_records and n != 0:
                for k, v in zip(ks, getattr(eng, "mfe_batch" if call == WINDOW else call)([seqs[k] for k in ks])):
                    out[k] = v
    return out


def pf_rows(eng, seq, cons, mfe_hints, banded=NEVER):
    """One record under several constraints (a string or None each), each scaled from its MFE hint (dcal/mol) -> a list of
    Engine.pf_long's dicts(dG, mean_bp_dist, centroid, centroid_dist): one pf_long_batch where that is the route, else a call
    per row; a window folds through fold_constrained."""
    call = _routed(pf_route, eng, len(seq), len(cons) > 1, banded)
    if call == "pf_long_batch":
        return eng.pf_long_batch([seq] * len(cons), cons, mfe_hints)  # in the same launches; each row is pf_long's bit for bit
    if call != WINDOW:
        return [getattr(eng, call)(seq, c, mfe_hint=h) for c, h in zip(cons, mfe_hints)]
    out = []
    for c in cons:
        r = eng.fold_constrained([seq], ["." * len(seq) if c is None else c], mfe=False)
        out.append({k: (r[k][0] if k == "centroid" else float(r[k][0])) for k in r})
    return out


def pf(eng, seq, cons=None, mfe_hint=None, banded=NEVER):
    """pf_rows of one row -> its dict"""
    return pf_rows(eng, seq, [cons], [mfe_hint], banded)[0]


def pf_probs(eng, seq, cons=None, mfe_hint=None, cutoff=0.01):
    """One record under the resident span -> Engine.pf_banded_probs's dict: pf_banded's plus the unpaired probabilities, the
    positional entropies and the sparse pair list.  The banded policy is ALWAYS (the probabilities leave the device from
    banded tables only; a span of at least the record's length gives the unrestricted ones), so the route is pf_route's
    banded one with the probabilities asked for; a library without sf_pf_banded_probs is a ScanFoldHipError."""
    call = _routed(pf_route, eng, len(seq), False, ALWAYS) + "_probs"
    if not getattr(eng, "has_" + call)():
        raise _lib.ScanFoldHipError("base-pair probabilities of a whole record need sf_%s, which this library (%s) does not "
                                    "export" % (call, getattr(eng.lib, "_name", "?")))
    return getattr(eng, call)(seq, cons, mfe_hint=mfe_hint, cutoff=cutoff)


def pf_mea(eng, seq, cons=None, mfe_hint=None, cutoff=0.01, gamma=1.0):
    """pf_probs with the maximum-expected-accuracy structure of its list (Engine.pf_banded_mea's dict: pf_banded_probs's plus
    mea and mea_score), on the same route: pf_route's banded one, the policy ALWAYS.  A library without sf_pf_banded_mea is a
    ScanFoldHipError."""
    call = _routed(pf_route, eng, len(seq), False, ALWAYS) + "_mea"
    if not getattr(eng, "has_" + call)():
        raise _lib.ScanFoldHipError("the maximum-expected-accuracy structure of a whole record needs sf_%s, which this library "
                                    "(%s) does not export" % (call, getattr(eng.lib, "_name", "?")))
    return getattr(eng, call)(seq, cons, mfe_hint=mfe_hint, cutoff=cutoff, gamma=gamma)
