"""The long-range-interaction (k-mer duplex) scan of ScanFold.py --lri (ScanFold.py:769-1034) on the HIP engine.

The reference folds every pair of k-mers more than kmer+3 apart with RNA.duplexfold from a Python double loop and, for
every pair below the cutoff, 101 more for a z-score.  Here the all-pairs scan is one device call that returns only the
pairs below the cutoff (Engine.lri_scan), their structures come from Engine.duplex_batch and their backgrounds from
Engine.lri_background; what is left on the host is the reference's bookkeeping of coordinates and its row format.

Quirks of the reference that are reproduced (DESIGN.md "Duplex folds"):
  * the outer loop runs one k-mer further than the inner one, so the last strand 1 is kmer-1 nucleotides long (:774,780);
  * the "native" energy of the z-score is a fold against a SHUFFLED k-mer, like every other element (ScanFoldFunctions.py:820);
  * `start_sequence_*` (:807-808) are computed and never used;
  * the base-pair list of a duplex that forms UPSTREAM of the k-mer is empty: the reference fills `rev_base_pairs` for it but
    walks `base_pairs`, which only the downstream branch fills (:892,933).
Not reproduced: the continuation into the Fold stage (:1027-1034 onwards), which upstream cannot run in general — see README.md.
"""
from . import _lib
from . import functions as sff
from .RNA import _f32

HEADER = "%s\t%s\t%s\t%s\t%s\t%s\n" % ("Coordinates(K-mer)", "Coordinates(Duplex)", "Sequence", "Structure", "z-score", "MFE")
WARNING = "WARNING! Using experimental LRI fuction. This has not been extensively tested, you may experience errors."


def hit_record(frag, dup_frag, j_win, k_win, energy_dcal, i, j, structure):
    """The reference's fields of one folded pair (ScanFold.py:786-811), without the z-score."""
    left, right = structure.split("&")
    n0, n1 = len(left), len(right)
    first0 = j_win + 1 + i - n0
    return dict(
        j_win=int(j_win), k_win=int(k_win), i=int(i), j=int(j),
        duplex_0_range="%d-%d" % (first0, j_win + i),
        duplex_1_range="%d-%d" % (k_win + j, k_win + j + n1 - 1),
        coordinates=list(range(first0, j_win + i + 1)) + ["&"] + list(range(k_win + j, k_win + j + n1)),
        sequence=frag[i - n0:i] + "&" + dup_frag[j - 1:j + n1 - 1],
        structure=structure,
        duplex_mfe=round(_f32(energy_dcal), 2),
    )


def check_lri_args(kmer, kmer_step_size):
    """refuse, before anything is scanned, what the engine cannot fold"""
    if not 2 <= int(kmer) <= _lib.SF_DUPLEX_MAX_LEN:
        raise ValueError("--kmer must be between 2 and %d (the longest strand the duplex kernels fold), not %d"
                         % (_lib.SF_DUPLEX_MAX_LEN, int(kmer)))
    if int(kmer_step_size) < 1:
        raise ValueError("--kmer_step_size must be at least 1, not %d" % int(kmer_step_size))


def lri_scan(seq, kmer=20, kmer_step_size=1, lri_cutoff=-25, randomizations=100, type="mono", engine=None, seed=0,
             max_hits=1 << 20):
    """-> the hit records of ScanFold.py:785-829 in the reference's order (by j_win, then k_win), each with
    `cofold_zscore` and `energy_list`; only those with cofold_zscore < 10 (:822).  lri_cutoff in kcal/mol."""
    eng = engine if engine is not None else _lib.get_engine()
    if type not in ("di", "mono"):
        raise ValueError('Shuffle type not properly designated; please input "di" or "mono"')
    kmer, step, r = int(kmer), int(kmer_step_size), int(randomizations)
    check_lri_args(kmer, step)
    seq = str(seq)
    # round(energy, 2) < lri_cutoff with energy = (float)Emin / 100  <=>  Emin < 100 * lri_cutoff: two decimals of a value
    # that is an integer number of hundredths round back to that integer
    cutoff_dcal = int(round(float(lri_cutoff) * 100))
    found = eng.lri_scan(seq, kmer, step, cutoff_dcal, max_hits=max_hits)
    if len(found) == 0:
        return []
    frags = [seq[h["j_win"]:h["j_win"] + kmer] for h in found]
    dups = [seq[h["k_win"]:h["k_win"] + kmer] for h in found]
    folded = eng.duplex_batch(frags, dups)
    kind = _lib.SHUFFLE_DI if type == "di" else _lib.SHUFFLE_MONO
    bg = eng.lri_background(seq, kmer, found["j_win"], found["k_win"], r, kind, seed)
    hits = []
    for x, h in enumerate(found):
        if int(folded["energy"][x]) != int(h["energy"]):
            raise _lib.ScanFoldHipError("LRI scan and duplex fold disagree on k-mers %d / %d" % (h["j_win"], h["k_win"]))
        rec = hit_record(frags[x], dups[x], h["j_win"], h["k_win"], h["energy"], h["i"], h["j"], folded["structure"][x])
        rec["energy_list"] = energy_list(bg[x])
        rec["cofold_zscore"] = round(sff.zscore_function(rec["energy_list"], r), 2)
        if rec["cofold_zscore"] < 10:
            hits.append(rec)
    return hits


def energy_list(row_dcal):
    """duplex.energy of a background row: (float)Emin / 100; two strands without a pair give ViennaRNA's (float)INF / 100."""
    return [_f32(10000000 if int(v) == _lib.SF_DUPLEX_NONE else int(v)) for v in row_dcal]


def lri_row(hit):
    return "%s\t%s\t%s\t%s\t%f\t%f\n" % (hit["duplex_0_range"], hit["duplex_1_range"], hit["sequence"], hit["structure"],
                                       hit["cofold_zscore"], hit["duplex_mfe"])


def write_lri(path, hits):
    with open(path, "w") as w:
        w.write(HEADER)
        for h in hits:
            w.write(lri_row(h))


def _pair_positions(structure):
    """1-based string positions [open, close, open, close, ...] of a duplex structure's pairs, by opening position"""
    opens = [x + 1 for x, ch in enumerate(structure) if ch == "("]
    closes = [x + 1 for x, ch in enumerate(structure) if ch == ")"]
    out = []
    for depth, o in enumerate(opens):  # the d-th '(' from the left closes with the d-th ')' from the right
        out += [o, closes[len(closes) - 1 - depth]]
    return out


def lri_pairs(hit):
    """The base pairs ScanFold.py:831-1015 derives from a hit, as (lb, lbp_coord, rb, rbp_coord) tuples in its order.
    A duplex downstream of the k-mer lists its pairs from the outermost inwards.  One UPSTREAM of it (first coordinate
    larger than the last) lists none: the reference numbers the pairs of the flipped structure there, but then walks the
    list only the downstream branch fills."""
    coords, sequence = hit["coordinates"], hit["sequence"]
    if coords[0] < coords[-1]:
        pos = _pair_positions(hit["structure"])
        return [(sequence[pos[x] - 1], coords[pos[x] - 1], sequence[pos[x + 1] - 1], coords[pos[x + 1] - 1])
                for x in range(0, len(pos), 2)]
    return []
