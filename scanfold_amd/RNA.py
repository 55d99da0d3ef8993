"""A minimal `RNA`-shaped facade over the HIP engine — just the names ScanFold calls.

reference call sites: RNA.md() ScanFold-Scan.py:70, ScanFold.py:212; RNA.fold_compound(seq, md) Scan:382;
fc.mfe() :385; fc.pf() :383; RNA.pf_fold(seq) :384; fc.centroid() :388; fc.mean_bp_distance() :389;
RNA.fold(seq) :245.  Energies come back as ViennaRNA returns them: (float)dcal / 100 widened to a Python float.
md.max_bp_span (ScanFold.py:214-215) is honoured (sf_set_max_bp_span).
md.temperature other than 37 needs a parameter set with enthalpy tables (params.load_par of a real .par file).
fc.hc_add_from_db and fc.sc_add_SHAPE_deigan (ScanFold-Scan.py:410; ScanFold.py:512,534) are provided through
sf_fold_constrained.  RNA.duplexfold(s1, s2) (ScanFold.py:785; ScanFoldFunctions.py:824) folds through sf_duplex_batch.
Not provided: plotting, Zarringhalam soft constraints (upstream's call fails too).
Sequences longer than SF_MAX_W (400 nt, the window kernels' limit) fold with fc.mfe() / RNA.fold as whole records,
hc_add_from_db included (ScanFold.py --global_refold, :1509-1547).  Which entry point they reach is scanfold_amd.whole's
decision, under its AUTO policy ("Routes of the whole-record folds"): full tables up to 32 767 nt, banded
tables under md.max_bp_span (the same bytes) for a longer record or one at least four spans long.  Their partition
function, centroid and mean base-pair distance exist in the engine (functions.rna_refold) but this facade does not route
to them yet: fc.pf() / fc.centroid() / fc.mean_bp_distance() raise NotImplementedError, as does the SHAPE term, which
does not exist past 400 nt.
The model is global state of the engine, like RNA's md defaults: Engine.md_span is the span this facade last made resident,
and a fold_compound changes the engine's span only when its model's differs from that record.
"""
import numpy as np

from . import _lib, whole


class md:
    def __init__(self):
        self.temperature = 37.0
        self.max_bp_span = -1
        self.dangles = 2


def _check_md(model):
    eng = _lib.get_engine()
    eng.set_temperature(float(model.temperature) if model is not None else 37.0)
    span = getattr(model, "max_bp_span", -1) if model is not None else -1
    span = int(span) if span not in (None, -1) and int(span) > 0 else 0
    if span != eng.md_span:  # the model is global state of the engine, like RNA's md defaults
        eng.set_max_bp_span(span)
        eng.md_span = span
    return eng


def _f32(dcal):
    return float(np.float32(dcal) / np.float32(100.0))


def deigan_pseudo_energies(reactivities, m, b, n):
    """vrna_sc_add_SHAPE_deigan [EXT]: position i (1-based) gets m*ln(reactivity[i] + 1) + b kcal/mol, 0 where the
    reactivity is negative (missing data); stored as (int)roundf(x * 100) dcal/mol.  The C function reads the vector
    1-BASED (index 0 is a dummy, as in ViennaRNA's own Python test the reference cites, ScanFold.py:219-221), and
    ScanFold passes a 0-based window slice (ScanFold.py:523,534), so upstream applies reactivity k+1 to nucleotide k and
    reads one element past the end for the last nucleotide.  That shift is reproduced here; the out-of-range element
    counts as missing data.  -> int32 array of n pseudo-energies (0-based)."""
    import math
    vals = [float(v) for v in reactivities]
    out = np.zeros(n, dtype=np.int32)
    for i in range(1, n + 1):
        r = vals[i] if i < len(vals) else -999.0
        x = 0.0 if r < 0 else m * math.log(r + 1.0) + b
        v = float(np.float32(x * 100.0))
        out[i - 1] = int(math.copysign(math.floor(abs(v) + 0.5), v))  # roundf: halves away from zero
    return out


class fold_compound:
    def __init__(self, sequence, model=None):
        self.sequence = str(sequence)
        self._model = model
        self._eng = _check_md(model)
        self._pf = None
        self._hc = None   # dot-bracket hard constraint (hc_add_from_db)
        self._sc = None   # Deigan pseudo-energies, int32 dcal per nucleotide (sc_add_SHAPE_deigan)

    def hc_add_from_db(self, constraint, options=None):
        """fc.hc_add_from_db(window_constraints) (ScanFold-Scan.py:410; ScanFold.py:512): '.', 'x', '|', '<', '>', '(' ')'
        with ViennaRNA's default (non-enforcing) meaning, see include/scanfold_hip.h: sf_fold_constrained."""
        constraint = str(constraint)
        if len(constraint) != len(self.sequence):
            raise ValueError("constraint string and sequence differ in length")
        self._hc = constraint
        self._pf = None
        return 1

    def sc_add_SHAPE_deigan(self, reactivities, m, b, options=None):
        """fc.sc_add_SHAPE_deigan(window_react_list, slope, intercept) (ScanFold.py:534,539)."""
        self._sc = deigan_pseudo_energies(reactivities, float(m), float(b), len(self.sequence))
        return 1

    def sc_add_SHAPE_zarringhalam(self, reactivities, b=None, default_value=None, shape_conversion=None, options=None):
        """ScanFold.py:536 calls this with ONE argument; ViennaRNA's binding needs b, default_value and the conversion
        string as well, so upstream's --shapeZ path ends in a TypeError.  Same here."""
        if b is None or default_value is None or shape_conversion is None:
            raise TypeError("sc_add_SHAPE_zarringhalam() missing required arguments: b, default_value, shape_conversion")
        raise NotImplementedError("Zarringhalam soft constraints are not implemented by the HIP engine")

    def mfe(self):
        self._eng = _check_md(self._model)
        e, db = whole.fold(self._eng, self.sequence, self._hc, whole.AUTO, self._sc)
        return db, _f32(e)

    def pf(self):
        """-> (structure string, ensemble free energy).  The string is the centroid structure, not
        ViennaRNA's pair-propensity string (ScanFold discards it, ScanFold-Scan.py:383)."""
        self._eng = _check_md(self._model)
        whole.pf_route(len(self.sequence), self._eng.max_bp_span, banded=whole.AUTO)  # refuses a whole record
        if self._sc is not None:
            raise NotImplementedError("partition function with SHAPE soft constraints (the reference calls fc.pf() "
                                      "before sc_add_SHAPE_*, ScanFold.py:525-539)")
        if self._hc is not None:
            r = self._eng.fold_constrained([self.sequence], [self._hc], None, mfe=False)
        else:
            r = self._eng.pf_batch([self.sequence])
        self._pf = r
        return r["centroid"][0], float(r["dG"][0])

    def centroid(self):
        if self._pf is None:
            self.pf()
        return self._pf["centroid"][0], float(self._pf["centroid_dist"][0])

    def mean_bp_distance(self):
        if self._pf is None:
            self.pf()
        return float(self._pf["mean_bp_dist"][0])


def fold(sequence):
    return fold_compound(sequence).mfe()


def pf_fold(sequence):
    return fold_compound(sequence).pf()


class duplexT:
    """What RNA.duplexfold returns: .energy (kcal/mol), .structure ("((.&.))"), .i (3' end of the strand-1 part, 1-based),
    .j (5' end of the strand-2 part).  Two strands that cannot form a pair: ViennaRNA leaves its minimum at INF, so .energy
    is (float)INF / 100 = 100000.0, with structure "&" and i = j = 0 here."""

    def __init__(self, energy, structure, i, j):
        self.energy, self.structure, self.i, self.j = energy, structure, i, j

    def __repr__(self):
        return "duplexT(energy=%r, structure=%r, i=%r, j=%r)" % (self.energy, self.structure, self.i, self.j)


def duplexfold(s1, s2):
    """RNA.duplexfold(s1, s2): the minimum-energy duplex of two strands of at most SF_DUPLEX_MAX_LEN nucleotides (only
    inter-strand pairs), at the engine's resident model (37 C unless a fold_compound with another md was made before)."""
    eng = _lib.get_engine()
    r = eng.duplex_batch([str(s1)], [str(s2)])
    e = int(r["energy"][0])
    return duplexT(_f32(10000000 if e == _lib.SF_DUPLEX_NONE else e), r["structure"][0], int(r["i"][0]), int(r["j"][0]))
