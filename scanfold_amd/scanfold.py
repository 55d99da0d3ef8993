"""ScanFold.py's scan stage + Fold stage on the HIP engine (the combined driver).

Restates the scan section of /root/reference/ScanFold.py (:420-757) — the ScanFoldFunctions flavour of the hot loop:
  z-score with the SAMPLE standard deviation and 0.0 when it vanishes      ScanFoldFunctions.py:741-751
  an eleventh column, the window's GC content                               ScanFold.py:433,685; SFF:1023-1036
  folds at md.temperature incl. the shuffles                                SFF:774-789  (ScanFold-Scan.py's differ, F8)
  md.max_bp_span = --span                                                   ScanFold.py:214-215
  --constraints: constrained native fold; --react: Deigan SHAPE term for the MFE only   ScanFold.py:508-544
and then feeds the windows straight into the Fold stage (scanfold_amd.fold; ScanFold.py:564-677,1036-1453) without a
TSV round trip; the pair tabulation of that stage runs on the GPU (sf_tabulate_pairs).  Output: `<name>.win_W.stp_S.rnd_R.shfl_T.out` (the scan table, ScanFold.py:381,685) and the Fold
stage's files with the prefix `<that>.ScanFold.`, then the dot-bracket files (makedbn) and the motif extraction /
refolds of ScanFold.py:1582-1776 (scanfold_amd.motifs: `<that>.ExtractedStructures.gff3`, `<that>_motif_<n>.dbn/.ct`).
--global_refold folds the whole record three times after the dbn files are written (ScanFold.py:1509-1547): unconstrained,
then with the -1 and the -2 filter's dot-bracket lines as hard constraints (whole-record folds, routed by scanfold_amd.whole
as the RNA facade routes them), into `<that>.<--dbn_file_path>` and `<that>.AllDBN.txt`.  ScanFold.py's per-record
directories and IGV wig exports are not reproduced.
--global_span N (not upstream) runs those three folds under max bp span N in banded tables (sf_fold_banded), and
--global_ensemble_banded adds their ensembles from the banded partition function (sf_pf_banded), at any record length, and
--global_bpp CUTOFF with it their base pairs with probability >= CUTOFF and positional entropy tracks (sf_pf_banded_probs),
and --global_mea GAMMA with that their maximum-expected-accuracy structures (sf_pf_banded_mea; RNAfold -p --MEA GAMMA).
--global_zscore (not upstream) z-scores the whole record against shuffles of itself (one batched whole-record fold,
sf_fold_long_batch) into `<that>.global_zscore.txt`; --global_zscore_span N (not upstream) does so under max bp span N in
banded tables (one sf_fold_banded_batch: linear in the record's length, records past 32767 nt).
--lri replaces the window scan by the k-mer duplex scan (ScanFold.py:391-393,421,769-1034; scanfold_amd.lri): it writes
`<that>.LRI.out`, reports the number of hits and stops — upstream's continuation into the Fold stage is not runnable in
general (README.md) and is not reproduced.
"""
import argparse
import os
import statistics
import sys

import numpy as np

from . import _lib, fold as foldmod
from . import functions as sff
from . import scan as scanmod
from . import motifs as motifmod
from . import whole, writers


def header_line(read_name):
    return ("i\tj\tTemperature\tNative_dG\tZ-score\tP-score\tEnsembleDiversity\tSequence\tStructure\tCentroid\t"
            + read_name + "\n")


def zscores_rows_sff(E, randomizations):
    """zscore_function of ScanFoldFunctions.py:741-751 for every row of E (n, r+1), rounded as the caller does
    (round(z, 2) on a Python float).  The `statistics` module works in exact rational arithmetic, numpy in floating
    point; the two can differ in the last bits of z, which only matters when z sits on a rounding boundary — those
    rows (and the ones whose deviation vanishes) are recomputed with the reference's own calls."""
    E = np.asarray(E, dtype=np.float64)
    n = len(E)
    if E.shape[1] < 2:
        raise statistics.StatisticsError("variance requires at least two data points")
    sd = E.std(axis=1, ddof=1)
    if randomizations > 1:
        mean = E[:, 1:randomizations].mean(axis=1)
    else:
        raise statistics.StatisticsError("mean requires at least one data point")
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (E[:, 0] - mean) / sd
    frac = np.abs(z * 100.0 - np.round(z * 100.0))
    exact_rows = np.nonzero(~np.isfinite(z) | (np.abs(frac - 0.5) < 1e-6) | (sd < 1e-9))[0]
    out = [round(v, 2) for v in z.tolist()]
    for k in exact_rows.tolist():
        out[k] = round(sff.zscore_function([float(v) for v in E[k]], randomizations), 2)
    return out


def gc_contents(tseq, starts, W):
    return [sff.get_gc_content(tseq[i:i + W]) for i in starts]


def scan_rows(seq, W, step, r, shuffle_type, temperature=37, engine=None, seed=0, constraints=None, reactivities=None,
              slope=0.8, intercept=-0.2, unbalanced="error"):
    """-> (rows, table): the TSV rows of ScanFold.py's `.out` file and the in-memory ScanTable of ALL windows."""
    from . import RNA
    eng = engine if engine is not None else _lib.get_engine()
    if shuffle_type not in ("di", "mono"):
        raise ValueError('Shuffle type not properly designated; please input "di" or "mono"')
    eng.set_temperature(int(temperature))
    tseq = scanmod.transcribe(seq)
    starts = scanmod.window_starts(len(seq), W, step)
    n_win = len(starts)
    kind = _lib.SHUFFLE_DI if shuffle_type == "di" else _lib.SHUFFLE_MONO
    plain = constraints is None and reactivities is None

    def work(w0, nw):
        if plain:
            return eng.scan(seq, W, step, w0, nw, r, kind, seed, raw=True)
        en = eng.scan(seq, W, step, w0, nw, r, kind, seed, _lib.SCAN_NO_PF | _lib.SCAN_NO_TRACE, raw=True)["energies"]
        wins = scanmod._window_rows(tseq, W, step, w0, nw)
        if constraints is not None:  # hc_add_from_db, then mfe and pf (ScanFold.py:508-520)
            cons = scanmod._window_rows(constraints, W, step, w0, nw)
            if unbalanced == "ignore":
                cons = scanmod._drop_unmatched_brackets(cons)
            fc = eng.fold_constrained(wins, cons)
            return dict(energies=en, native=fc["mfe"], structure=fc["structure"], centroid=fc["centroid"],
                        ens_div=fc["mean_bp_dist"])
        # SHAPE: pf first (unconstrained), then the Deigan term, then mfe (ScanFold.py:522-544)
        pf = eng.pf_batch(wins)
        sc = np.stack([RNA.deigan_pseudo_energies(reactivities[starts[w0 + t] + 1:starts[w0 + t] + W + 1], slope,
                                                  intercept, W) for t in range(nw)])
        fc = eng.fold_constrained(wins, None, sc, pf=False)
        return dict(energies=en, native=fc["mfe"], structure=fc["structure"], centroid=pf["centroid"],
                    ens_div=pf["mean_bp_dist"])

    rows, t_mfe, t_z, t_p, t_ed, t_struct = [], [], [], [], [], []
    for w0, res in scanmod._engine_chunks(work, 0, n_win):
        sub = starts[w0:w0 + len(res["ens_div"])]
        E = scanmod.dcal_to_float(res["energies"])
        nat = E[:, 0] if "native" not in res else scanmod.dcal_to_float(res["native"])
        mfe = [round(v, 2) for v in nat.tolist()]
        zs = zscores_rows_sff(E, r)
        ps = [round(v, 2) for v in scanmod.sfn.pscores_rows(E).tolist()]
        eds = [round(v, 2) for v in np.asarray(res["ens_div"], dtype=np.float64).tolist()]
        structs = scanmod._text_rows(res["structure"], W)
        cens = scanmod._text_rows(res["centroid"], W)
        gcs = gc_contents(tseq, sub, W)
        t = str(int(temperature))
        for k, i in enumerate(sub):
            frag = tseq[i:i + W]
            if frag == scanmod.ALL_N_120:  # ScanFold.py:486-492
                rows.append("%d\t%d\t%s\t0\t#DIV/0\t0\t0\t%s\t%s\t%s\t%s\n" % (i + 1, i + W, t, frag, scanmod.DOTS_120,
                                                                               scanmod.DOTS_120, str(gcs[k])))
                mfe[k], zs[k], ps[k], eds[k], structs[k] = 0.0, float("nan"), 0.0, 0.0, scanmod.DOTS_120
                continue
            rows.append("%d\t%d\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n" % (i + 1, i + W, t, str(mfe[k]), str(zs[k]), str(ps[k]),
                                                                           str(eds[k]), frag, structs[k], cens[k], str(gcs[k])))
        t_mfe += mfe; t_z += zs; t_p += ps; t_ed += eds; t_struct += structs
    table = foldmod.ScanTable("", [i + 1 for i in starts], t_mfe, t_z, t_ed, [tseq[i:i + W] for i in starts], t_struct)
    table.pvalues = t_p  # the fourth metric list of ScanFold.py (:691): only the scan-pvalue wig track reads it
    return rows, table


def read_reactivities(path):
    """getShapeDataFromFile (ScanFold.py:218-262): 1-based list with -999.0 at index 0 and for missing positions / NA."""
    vec = [-999.0]
    count = 1
    with open(path, "r") as f:
        lines = f.read().splitlines()
    ncol = len(lines[0].split("\t"))
    if ncol not in (2, 3):
        raise TypeError("exceptions must derive from BaseException")  # upstream: raise("Trouble parsiging reactivity data")
    for line in lines:
        parts = line.split("\t")
        pos = int(parts[0])
        value = parts[2] if ncol == 3 else parts[1]
        if value == "NA":
            value = -999
        if pos != count:
            vec.extend([-999.0] * (pos - count))
            count = pos
        vec.append(float(value))
        count += 1
    return vec


def global_refold(seq, name, outname, temperature, dbn_file_path="AllDBN-global_refold.txt", ensemble=False, span=0,
                  ensemble_banded=False, bpp=None, mea=None):
    """ScanFold.py:1509-1547 (--global_refold): a fresh RNA.md() at md.temperature = int(-t) — no --span, exactly as
    upstream — folds the whole record unconstrained and with line 3 of `<outname>.ScanFold.-1.dbn` / `.-2.dbn` as
    hc_add_from_db constraint, and writes the three records to `<outname>.<dbn_file_path>`; `<outname>.AllDBN.txt` is the
    three dbn files concatenated (upstream's `cat`).  Upstream hands the constraint line over with its trailing newline;
    what ViennaRNA makes of that extra character could not be checked against ViennaRNA itself, so it is stripped here
    (the constraint is exactly as long as the record).  The dbn files cover the scanned stretch only, positions 1 .. the
    last window's end; when the windows stop short of the record's end the line is padded with '.' (no ScanFold pair
    there, so no constraint) to the record's length.
    The engine's model (base-pair span, temperature, and the RNA facade's record of the span) is put back exactly as it
    was, also when a fold raises (Engine.saved_model): the stages after this one, and the next records, fold as they would
    without the flag.  Which entry point each fold reaches is scanfold_amd.whole's decision; the flags only set the policy.
    ensemble (--global_ensemble, not upstream): the partition function of the same three folds in full tables (one
    Engine.pf_long_batch call past SF_MAX_W where the library has it, else Engine.pf_long three times: the same numbers;
    scaled from each fold's MFE) into `<outname>.<dbn_file_path minus .txt>.ensemble.txt`, three records of a header line
    (ensemble free energy, ED = mean base-pair distance to 2 decimals, centroid distance), the sequence and the centroid.
    span (--global_span N, not upstream): the three folds run under max_bp_span = N in banded tables (Engine.fold_banded:
    memory and work linear in the record's length, records past SF_MAX_LONG), and the header lines gain " span=N".
    ensemble_banded (--global_ensemble_banded, not upstream; needs span): the same ensemble file from Engine.pf_banded, the
    partition function under the span in banded tables, each fold's MFE as hint: any record fold_banded takes, where
    --global_ensemble stops at SF_MAX_LONG.  Its header lines carry " span=N" too.
    bpp (--global_bpp CUTOFF, not upstream; needs ensemble_banded): the three ensembles go through Engine.pf_banded_probs,
    whose four classic values are pf_banded's bit for bit, so the ensemble file is the same bytes; for each fold (tags
    full, -1, -2) two more files: `<outname>.global_refold.<tag>.bpp.txt`, a header line "i\tj\tp span=N" and one
    "%d\t%d\t%.6g" line per pair with p >= CUTOFF, ascending in (i, j) and 1-based, and
    `<outname>.global_refold.<tag>.entropy.wig`, the positional entropy in bits, one value per nucleotide.
    mea (--global_mea GAMMA, not upstream; needs bpp): the three ensembles go through Engine.pf_banded_mea, whose other
    values are pf_banded_probs's bit for bit, so every file above is the same bytes; each fold gains
    `<outname>.global_refold.<tag>.mea.dbn`: a header ">NAME TAG MEA gamma=%g cutoff=%g span=%d score=%.2f", the sequence,
    and the maximum-expected-accuracy structure of the listed pairs (RNAfold -p --MEA GAMMA)."""
    from . import RNA
    span = int(span or 0)
    tail = " span=%d" % span if span > 0 else ""
    cons = []
    for tag in ("-1", "-2"):
        with open(outname + ".ScanFold." + tag + ".dbn") as f:
            line = f.readlines()[2].rstrip("\r\n")
        cons.append(line + "." * max(0, len(seq) - len(line)))
    eng = _lib.get_engine()
    with eng.saved_model():
        eng.set_max_bp_span(span)  # (the scan's --span is engine state; the fresh md has none, or --global_span's)
        eng.md_span = span
        eng.set_temperature(float(int(temperature)))
        (e1, s1), (e2, s2), (e0, s0) = ((RNA._f32(e), db) for e, db in (
            whole.fold(eng, seq, c, whole.ALWAYS if span > 0 else whole.AUTO) for c in (cons[0], cons[1], None)))
        ens = []
        hints = [int(round(e * 100)) for e in (e0, e1, e2)]
        if ensemble_banded and bpp is not None and mea is not None:
            ens = [whole.pf_mea(eng, seq, c, h, bpp, mea) for c, h in zip([None, cons[0], cons[1]], hints)]
        elif ensemble_banded and bpp is not None:
            ens = [whole.pf_probs(eng, seq, c, h, bpp) for c, h in zip([None, cons[0], cons[1]], hints)]
        elif ensemble or ensemble_banded:
            ens = whole.pf_rows(eng, seq, [None, cons[0], cons[1]], hints, whole.ALWAYS if ensemble_banded else whole.NEVER)
    with open(outname + "." + dbn_file_path, "w") as w:
        w.write(">" + str(name) + "\tGlobal Full MFE=" + str(e0) + tail + "\n" + seq + "\n" + s0 + "\n")
        w.write(">" + str(name) + "\tRefolded with -1 constraints MFE=" + str(e1) + tail + "\n" + seq + "\n" + s1 + "\n")
        w.write(">" + str(name) + "\tRefolded with -2 constraints MFE=" + str(e2) + tail + "\n" + seq + "\n" + s2 + "\n")
    if ensemble or ensemble_banded:
        ens_tail = tail if ensemble_banded else ""
        stem = dbn_file_path[:-4] if dbn_file_path.endswith(".txt") else dbn_file_path
        with open(outname + "." + stem + ".ensemble.txt", "w") as w:
            for label, r in zip(("Global Full", "Refolded with -1 constraints", "Refolded with -2 constraints"), ens):
                w.write(">%s\t%s ensemble dG=%.2f ED=%.2f centroid distance=%.2f%s\n%s\n%s\n"
                        % (name, label, r["dG"], r["mean_bp_dist"], r["centroid_dist"], ens_tail, seq, r["centroid"]))
    if ensemble_banded and bpp is not None:
        for tag, r in zip(("full", "-1", "-2"), ens):
            with open(outname + ".global_refold." + tag + ".bpp.txt", "w") as w:
                w.write("i\tj\tp" + tail + "\n")
                w.write("".join("%d\t%d\t%.6g\n" % (i, j, p) for i, j, p in r["pairs"].tolist()))
            writers.write_wig(r["entropy"].tolist(), 1, name, outname + ".global_refold." + tag + ".entropy.wig")
            if mea is not None:
                with open(outname + ".global_refold." + tag + ".mea.dbn", "w") as w:
                    w.write(">%s %s MEA gamma=%g cutoff=%g span=%d score=%.2f\n%s\n%s\n"
                            % (name, tag, mea, bpp, span, r["mea_score"], seq, r["mea"]))
    with open(outname + ".AllDBN.txt", "w") as w:
        for tag in ("no_filter", "-1", "-2"):
            with open(outname + ".ScanFold." + tag + ".dbn") as f:
                w.write(f.read())


GLOBAL_ZSCORE_HEADER = ("Name\tLength\tTemperature\tRandomizations\tShuffleType\tMFE\tShuffleMeanMFE\tShuffleStdevMFE\t"
                        "Z-score\tP-value\n")


def global_zscore(seq, name, outname, temperature, randomizations, shuffle_type, seed=0, span=0):
    """--global_zscore (not upstream): the z-score of the WHOLE record.  The unconstrained MFE of `seq` at int(-t) under the
    model of global_refold (no --span) against `randomizations` shuffles of it (`functions.scramble`, "di" or "mono"), folded
    together as `functions.energies` folds them — past 400 nt one batched whole-record fold (sf_fold_long_batch) — and turned
    into a z-score and p-value by `zscore_function` / `pvalue_function`, quirks included.  Writes `<outname>.global_zscore.txt`: a
    header line and one tab-separated row of name, length, temperature, randomizations, shuffle type, MFE, mean and sample
    standard deviation of the shuffles' MFEs, z-score, p-value, the numbers through str(round(x, 2)) as in the scan table.
    Cost: r + 1 folds of the whole record, O(L^3) each: tenths of a second at 1 kb, about twenty minutes at 30 kb with
    r = 100 by the single-fold time of DESIGN 4.4 (the batch's tables for such a record are one chunk per sequence).
    The shuffles draw from Python's `random` seeded with `seed`; the generator's state, and the engine's span, parameter
    set and temperature (Engine.saved_model), are put back as they were, also when a fold raises, so every other output of the
    run is the same with and without the flag.
    span (--global_zscore_span N, not upstream): the record and the same shuffles are folded under max_bp_span = N in banded
    tables, all r + 1 of them in one Engine.fold_banded_batch (sf_fold_banded_batch: B = min(N, L) fill launches for all of
    them, their exterior loops side by side), at a cost linear in the record's length and at any length up to
    SF_MAX_BANDED; the file gains a trailing column Span."""
    import random
    span = int(span or 0)
    eng = _lib.get_engine()
    state0 = random.getstate()
    try:
        random.seed(seed)
        shuffles = sff.scramble(seq, randomizations, shuffle_type)
    finally:
        random.setstate(state0)
    with eng.saved_model():
        eng.set_max_bp_span(span)  # (the scan's --span is engine state; the whole-record model has none, or this flag's)
        eng.set_temperature(int(temperature))
        E = sff._dcal_to_float(whole.fold_rows(eng, [seq] + shuffles, whole.ALWAYS if span > 0 else whole.NEVER))
    z = sff.zscore_function(E, randomizations)
    p = sff.pvalue_function(E, randomizations)
    row = [str(name), str(len(seq)), str(int(temperature)), str(randomizations), str(shuffle_type)]
    row += [str(round(x, 2)) for x in (E[0], statistics.mean(E[1:]), statistics.stdev(E[1:]), z, p)]
    header = GLOBAL_ZSCORE_HEADER
    if span > 0:
        header = header[:-1] + "\tSpan\n"
        row.append(str(span))
    with open(outname + ".global_zscore.txt", "w") as w:
        w.write(header)
        w.write("\t".join(row) + "\n")


def build_parser():
    p = argparse.ArgumentParser(description="ScanFold (scan + fold) on the MI355X HIP engine")
    p.add_argument('filename', type=str, help='input fasta')
    p.add_argument('--react', type=str, help='input SHAPE reactivity file')
    p.add_argument('-m', type=float, default=0.8, help='SHAPE slope value')
    p.add_argument('-b', type=float, default=-0.2, help='SHAPE intercept value')
    p.add_argument('--shapeD', action='store_true')
    p.add_argument('--shapeZ', action='store_true')
    p.add_argument('-f', type=int, default=-2, help='filter value')
    p.add_argument('-c', type=int, default=1, help='Competition (1 for disallow competition, 0 for allow; 1 by default)')
    p.add_argument('--name', type=str, default="UserInput", help='name of data being analyzed (chrom= of the wig tracks)')
    p.add_argument('--final_partners_wig', type=str, default="./IGV_BP_Zavg_metrics", help='final partners wig file path')
    p.add_argument('-s', type=int, default=1, help='step size')
    p.add_argument('-w', type=int, default=120, help='window size')
    p.add_argument('-r', type=int, default=100, help='randomizations')
    p.add_argument('-t', type=int, default=37, help='Folding temperature')
    p.add_argument('--type', type=str, default='mono', help='randomization type')
    p.add_argument('--print_random', action='store_true')
    p.add_argument('--algo', type=str, default='rnafold')
    p.add_argument('--constraints', type=str, help='optional | input constraint file')
    p.add_argument('--span', type=int, help='Max bp span')
    p.add_argument('--global_refold', action='store_true',
                   help='Global refold option. Refold full sequence using Zavg <-1 and <-2 base pairs')
    p.add_argument('--global_ensemble', action='store_true',
                   help='with --global_refold: also write ensemble free energy, ED and centroid of the three whole-record folds')
    p.add_argument('--global_span', type=int, default=None,
                   help='not in upstream ScanFold: with --global_refold, fold the whole record under this max bp span in banded '
                        'tables (memory and time linear in its length; records past 32767 nt)')
    p.add_argument('--global_ensemble_banded', action='store_true',
                   help='not in upstream ScanFold: with --global_refold and --global_span N, write the ensemble file of '
                        '--global_ensemble from the partition function under the span in banded tables (records past 32767 nt)')
    p.add_argument('--global_bpp', type=float, default=None, metavar='CUTOFF',
                   help='not in upstream ScanFold: with --global_ensemble_banded, also write the base pairs with probability '
                        '>= CUTOFF (0 < CUTOFF <= 1) and the positional entropy track of each of the three ensembles')
    p.add_argument('--global_mea', type=float, default=None, metavar='GAMMA',
                   help='not in upstream ScanFold: with --global_bpp, also write the maximum-expected-accuracy structure of each '
                        'of the three ensembles (RNAfold -p --MEA GAMMA; GAMMA > 0, larger values give more pairs)')
    p.add_argument('--global_zscore', action='store_true',
                   help='not in upstream ScanFold: z-score of the whole record (its MFE at -t, no --span, against -r shuffles of '
                        '--type seeded with --seed) into <output prefix>.global_zscore.txt; costs r + 1 whole-record folds')
    p.add_argument('--global_zscore_span', type=int, default=None,
                   help='not in upstream ScanFold: the z-score of --global_zscore under this max bp span, the record and its '
                        'shuffles folded together in banded tables (time linear in its length; records past 32767 nt); '
                        'the file gains a Span column')
    p.add_argument('--dbn_file_path', type=str, default="AllDBN-global_refold.txt",
                   help='file name (after the output prefix) of the global refold records')
    p.add_argument('--lri', action='store_true', help='scan for long range interactions (k-mer duplexes) instead of windows')
    p.add_argument('--kmer', type=int, default=20, help='size of k-mer for lri scan')
    p.add_argument('--kmer_step_size', type=int, default=1, help='step size of k-mer scan for lri')
    p.add_argument('--lri_cutoff', type=int, default=-25, help='duplex energy (kcal/mol) a k-mer pair must stay below')
    p.add_argument('--dont_fold', action='store_true', help='scan only')
    p.add_argument('--dont_extract', action='store_true', help='no motif extraction / refolds after the Fold stage')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--params', type=str, default=None)
    p.add_argument('--constraint-unbalanced', choices=("error", "ignore"), default="error")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.algo != "rnafold":
        raise NameError("name 'RNAstructure' is not defined")  # upstream's rnastructure backend is never imported (ScanFold.py:40,439)
    if args.c not in (0, 1):
        raise ValueError("-c must be 1 (no competition allowed) or 0 (competition allowed)")
    if args.global_refold and (args.c == 0 or args.dont_fold):
        # upstream scans first and then fails on the dbn files those modes never write
        raise ValueError("--global_refold refolds with the -1 / -2 dbn files of the Fold stage: not with -c 0 or --dont_fold")
    if args.global_ensemble and not args.global_refold:
        raise ValueError("--global_ensemble adds the partition function to the folds of --global_refold: give both")
    if args.global_ensemble_banded and (not args.global_refold or args.global_span is None):
        raise ValueError("--global_ensemble_banded is the ensemble of the folds of --global_refold under --global_span N: "
                         "give all three")
    if args.global_ensemble_banded and args.global_ensemble:
        raise ValueError("--global_ensemble and --global_ensemble_banded write the same file: give one of them")
    if args.global_mea is not None:
        if args.global_bpp is None:
            raise ValueError("--global_mea GAMMA folds the base-pair probabilities of --global_bpp into a structure: give both")
        if not (np.isfinite(args.global_mea) and args.global_mea > 0.0):
            raise ValueError("--global_mea GAMMA: a finite weight, GAMMA > 0")
        if args.lri:
            raise ValueError("--global_mea folds the record of a window scan: not with --lri")
    if args.global_bpp is not None:
        if not args.global_ensemble_banded:
            raise ValueError("--global_bpp CUTOFF lists the base-pair probabilities of the ensembles of "
                             "--global_ensemble_banded: give both")
        if not 0.0 < args.global_bpp <= 1.0:  # (a NaN fails both comparisons)
            raise ValueError("--global_bpp CUTOFF: a probability, 0 < CUTOFF <= 1")
        if args.lri:
            raise ValueError("--global_bpp lists the pairs of the record of a window scan: not with --lri")
    if args.global_span is not None and (not args.global_refold or args.global_span < 1):
        raise ValueError("--global_span N (N >= 1) sets the base-pair span of the folds of --global_refold: give both")
    lengths = []

    def past(route, *policy):
        """(name, length, limit) of the first record longer than the entry point whole.<route>(L, *policy) sends it to takes,
        or None: what is refused before any record is scanned.  The file is read once, by the first check that needs it."""
        if not lengths:
            lengths.extend((name, len(seq)) for name, seq in scanmod.read_fasta(args.filename))
        return next(((name, L, route(L, *policy).limit) for name, L in lengths if L > route(L, *policy).limit), None)

    if args.global_span is not None and (args.global_ensemble or args.global_zscore):
        hit = past(whole.pf_route if args.global_ensemble else whole.mfe_route, args.global_span, True, whole.NEVER)
        if hit:
            raise ValueError("--global_span: record %s has %d nt; %s stops at %d nt"
                             % (hit[0], hit[1], "--global_ensemble (the partition function in full tables; "
                                "--global_ensemble_banded has no such limit)" if args.global_ensemble
                                else "--global_zscore (the batched fold of the shuffles) has no banded form yet and", hit[2]))
    if args.global_ensemble_banded:
        hit = past(whole.pf_route, args.global_span, True, whole.ALWAYS)
        if hit:
            raise ValueError("--global_ensemble_banded: record %s has %d nt, banded folds stop at %d" % hit)
    if args.global_zscore and args.lri:
        raise ValueError("--global_zscore z-scores the record of a window scan: not with --lri")
    if args.global_zscore_span is not None:
        if args.global_zscore:
            raise ValueError("--global_zscore and --global_zscore_span write the same file: give one of them")
        if args.lri:
            raise ValueError("--global_zscore_span z-scores the record of a window scan: not with --lri")
        if args.global_zscore_span < 1:
            raise ValueError("--global_zscore_span N needs a base-pair span N >= 1")
        if args.type not in ("di", "mono"):
            raise ValueError('Shuffle type not properly designated; please input "di" or "mono"')
        hit = past(whole.mfe_route, args.global_zscore_span, True, whole.ALWAYS)
        if hit:
            raise ValueError("--global_zscore_span: record %s has %d nt, banded folds stop at %d" % hit)
    if args.global_zscore:
        if args.type not in ("di", "mono"):
            raise ValueError('Shuffle type not properly designated; please input "di" or "mono"')
        hit = past(whole.mfe_route, 0, True, whole.NEVER)
        if hit:
            raise ValueError("--global_zscore: record %s has %d nt, whole-record folds stop at %d" % hit)
    if args.lri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("--lri runs on one GPU: start it without a multi-process launcher")
        from . import lri as lrimod
        lrimod.check_lri_args(args.kmer, args.kmer_step_size)
    from . import params as _params
    eng = _lib.get_engine()
    eng.set_max_bp_span(args.span or 0)
    if args.params:
        eng.load_params(_params.load_par(args.params))
    W, step, r = int(args.w), int(args.s), int(args.r)
    for read_name, seq in scanmod.read_fasta(args.filename):
        seq = scanmod.transcribe(seq)
        if "-" in seq:
            raise TypeError("exceptions must derive from BaseException")  # upstream: raise("Gaps found in sequence...")
        outname = read_name + ".win_" + str(W) + ".stp_" + str(step) + ".rnd_" + str(r) + ".shfl_" + str(args.type)
        print("Output name=" + str(outname))
        if args.lri:  # replaces the window scan and everything after it (ScanFold.py:391-393,421,769-1034)
            print(lrimod.WARNING)
            print("Scanning for long range interactions...")
            hits = lrimod.lri_scan(seq, args.kmer, args.kmer_step_size, args.lri_cutoff, r, args.type, eng, args.seed)
            lrimod.write_lri(outname + ".LRI.out", hits)
            print("LRI Scan Complete: %d hits in %s.LRI.out" % (len(hits), outname))
            continue
        if len(seq) < W:
            print(read_name + " sequence is less than window size. Moving on to next entry.")
            continue
        cons = react = None
        if args.constraints is not None:
            print("Considering constraint input")
            cons = scanmod.read_constraints(args.constraints, len(seq))
        if args.react is not None:
            print("Considering SHAPE reactivity input")
            if args.shapeZ and not args.shapeD:
                raise TypeError("sc_add_SHAPE_zarringhalam() missing required arguments: b, default_value, shape_conversion")
            react = read_reactivities(args.react)
        rows, table = scan_rows(seq, W, step, r, args.type, args.t, eng, args.seed, cons, react, args.m, args.b,
                                args.constraint_unbalanced)
        with open(outname + ".out", "w") as w:
            w.write(header_line(read_name))
            w.writelines(rows)
        if not args.dont_fold:
            table.id = read_name
            # ScanFold.py tabulates every window (its inline loop has no dropped first row, unlike ScanFold-Fold.py)
            if args.c == 0:  # competition allowed: DP files + the track of the best partners, no CT / dbn / motifs (ScanFold.py:1454-1465)
                foldmod.fold(table, outname + ".ScanFold.", filt=int(args.f), bp_path=outname + ".ALL.bp", engine=eng,
                             competition=0)
            else:
                tab, res = foldmod.fold(table, outname + ".ScanFold.", filt=int(args.f), bp_path=outname + ".bp", engine=eng)
                for tag, label in (("no_filter", "NoFilter"), ("-1", "Zavg_-1"), ("-2", "Zavg_-2")):
                    writers.makedbn(outname + ".ScanFold." + tag, label)  # ScanFold.py:1487-1489
                # per-nucleotide mean z-score of the final partners, the track of the best partners (ScanFold.py:1491-1492)
                writers.write_wig_dict(res.fin_z.tolist(), args.final_partners_wig + "." + outname + ".wig", args.name, step)
                foldmod.write_bp(tab, res, outname + ".ALL.bp", tab.id, best=True)
            # the scanned sequence and the four per-window metric tracks (ScanFold.py:1494-1500)
            writers.write_fasta(seq, args.name + "." + outname + ".fa", args.name)
            zlist = [("#DIV/0" if z != z else z) for z in table.z.tolist()]  # (all-N windows, ScanFold.py:486-492)
            writers.write_wig(table.mfe.tolist(), step, args.name, outname + ".scan-MFE.wig")
            writers.write_wig(zlist, step, args.name, outname + ".scan-zscores.wig")
            writers.write_wig(table.pvalues, step, args.name, outname + ".scan-pvalue.wig")
            writers.write_wig(table.ed.tolist(), step, args.name, outname + ".scan-ED.wig")
            if args.global_zscore or args.global_zscore_span:
                print("Folding the full sequence and its shuffles for the global z-score...")
                global_zscore(seq, args.name, outname, args.t, r, args.type, args.seed, span=args.global_zscore_span or 0)
            if args.global_refold:
                print("Refolding full sequence using ScanFold results as constraints...")
                global_refold(seq, args.name, outname, args.t, args.dbn_file_path, ensemble=args.global_ensemble,
                              span=args.global_span or 0, ensemble_banded=args.global_ensemble_banded, bpp=args.global_bpp,
                              mea=args.global_mea)
            if args.c == 1 and not args.dont_extract:
                with open(outname + ".ScanFold.-2.dbn") as f:
                    line = f.readlines()[2]
                found = motifmod.extract_structures(line, seq)
                motifmod.refold_motifs(read_name, found, args.type, outname + ".ExtractedStructures.gff3",
                                       folder=motifmod.EngineFolder(args.t, args.algo), file_prefix=outname)
        elif args.global_zscore or args.global_zscore_span:
            global_zscore(seq, args.name, outname, args.t, r, args.type, args.seed, span=args.global_zscore_span or 0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
