"""Test helper: write a parameter set as a ViennaRNA "RNAfold parameter file v2.0" in the PUBLISHED file's layout —
free-energy section, then its `_enthalpies` twin, block comments before and after rows, dG / dH column pairs in
NINIO / ML_params / Misc and in the special-loop lists.  (The real rna_turner2004.par is absent from this machine;
this reproduces its format, not its numbers.)  Also: fully randomised parameter sets for the kernel tests
(random_params_full, boundary_params, random_enthalpies) and sequences with their special hairpins planted in them."""
import numpy as np

PAIRS = ["CG", "GC", "GU", "UG", "AU", "UA", "NS"]
INF = 10000000


def _tok(v, def_mask=False):
    if def_mask:
        return "DEF"
    return "INF" if v >= INF else ("-INF" if v <= -INF else str(int(v)))


def _rows(out, flat, per, mask=None, comments=None):
    flat = list(np.asarray(flat).reshape(-1))
    m = [False] * len(flat) if mask is None else list(np.asarray(mask).reshape(-1))
    for k in range(0, len(flat), per):
        line = " ".join("%6s" % _tok(v, d) for v, d in zip(flat[k:k + per], m[k:k + per]))
        if comments:
            line += "    /* %s */" % comments[(k // per) % len(comments)]
        out.append(line)


def par_text(rec, dH=None, def_fields=None):
    """rec / dH: numpy records of params.BLOB_DTYPE.  def_fields: {field: boolean mask} -> those entries become DEF."""
    def_fields = def_fields or {}
    out = ["## RNAfold parameter file v2.0", "",
           "/* This file contains energy parameters for RNA folding.            */",
           "/* written by tests/par_util.py in the layout of rna_turner2004.par */",
           "/* a comment that",
           "   spans two lines */", ""]
    mm = [("mismatch_hairpin", "mismatchH"), ("mismatch_interior", "mismatchI"),
          ("mismatch_interior_1n", "mismatch1nI"), ("mismatch_interior_23", "mismatch23I"),
          ("mismatch_multi", "mismatchM"), ("mismatch_exterior", "mismatchExt")]

    def both(name, emit):
        for suffix, r in (("", rec), ("_enthalpies", dH)):
            if r is None:
                continue
            out.append("# " + name + suffix)
            emit(r, def_fields if suffix == "" else {})
            out.append("")

    both("stack", lambda r, d: (out.append("/*  CG     GC     GU     UG     AU     UA     NS  */"),
                                 _rows(out, r["stack"][1:8, 1:8], 7, d.get("stack"), PAIRS)))
    for sec, field in mm:
        both(sec, lambda r, d, f=field: _rows(out, r[f][1:8], 5, d.get(f),
                                               ["%s,%s" % (p, b) for p in PAIRS for b in "NACGU"]))
    both("dangle5", lambda r, d: (out.append("/*  N      A      C      G      U  */"),
                                   _rows(out, r["dangle5"][1:8], 5, d.get("dangle5"), PAIRS)))
    both("dangle3", lambda r, d: (out.append("/*  N      A      C      G      U  */"),
                                   _rows(out, r["dangle3"][1:8], 5, d.get("dangle3"), PAIRS)))

    def int11(r, d):
        for a in range(1, 8):
            for b in range(1, 8):
                out.append("/* %s..%s */" % (PAIRS[a - 1], PAIRS[b - 1]))
                _rows(out, r["int11"][a, b], 5, None if "int11" not in d else d["int11"][a - 1, b - 1])
    both("int11", int11)

    def int21(r, d):
        for a in range(1, 8):
            for b in range(1, 8):
                for x in range(5):
                    out.append("/* %s.%s..%s */" % (PAIRS[a - 1], "NACGU"[x], PAIRS[b - 1]))
                    _rows(out, r["int21"][a, b, x], 5)
    both("int21", int21)

    def int22(r, d):
        for a in range(1, 7):
            for b in range(1, 7):
                for w in range(1, 5):
                    for x in range(1, 5):
                        out.append("/* %s.%s%s..%s */" % (PAIRS[a - 1], "NACGU"[w], "NACGU"[x], PAIRS[b - 1]))
                        _rows(out, r["int22"][a, b, w, x, 1:5, 1:5], 4)
    both("int22", int22)
    both("hairpin", lambda r, d: _rows(out, r["hairpin"], 10, d.get("hairpin")))
    both("bulge", lambda r, d: _rows(out, r["bulge"], 10))
    both("interior", lambda r, d: _rows(out, r["internal_loop"], 10))

    h = dH if dH is not None else np.zeros((), dtype=rec.dtype)
    out += ["# NINIO", "/* Ninio = MIN(max, m*|n1-n2| */", "/*       m   m_dH     max  */",
            "  %6d %6d %6d" % (rec["ninio"], h["ninio"], rec["max_ninio"]), ""]
    out += ["# ML_params", "/* F = cu*n_unpaired + cc + ci*loop_degree (+TermAU) */",
            "/*\t    cu\t    cu_dH\t    cc\t    cc_dH\t    ci\t    ci_dH  */",
            "\t%6d\t%6d\t%6d\t%6d\t%6d\t%6d" % (rec["MLbase"], h["MLbase"], rec["MLclosing"], h["MLclosing"],
                                               rec["MLintern"][1], h["MLintern"][1]), ""]
    out += ["# Misc", "/* all parameters are pairs of 'energy enthalpy' */",
            "/*    DuplexInit     TerminalAU   LXC  */",
            "   %d     %d     %d     %d     %.6f\t0.000000" % (rec["DuplexInit"], h["DuplexInit"], rec["TerminalAU"],
                                                              h["TerminalAU"], float(rec["lxc"])), ""]
    for sec, fseq, fe, fn in (("Triloops", "tri_seq", "tri_E", "n_tri"), ("Tetraloops", "tetra_seq", "tetra_E", "n_tetra"),
                              ("Hexaloops", "hexa_seq", "hexa_E", "n_hexa")):
        out.append("# " + sec)
        for k in range(int(rec[fn])):
            out.append("%s %6d %6d" % (bytes(rec[fseq][k]).rstrip(b"\0").decode(), rec[fe][k], h[fe][k]))
        out.append("")
    out += ["#END", ""]
    return "\n".join(out)


SF_FAST_MAXPARAM = 2500  # sf_mfe_fast.hip.h: a set with a finite entry beyond this goes to the int32 kernel at every width
SPECIAL_COUNTS = (0, 1, 7, 8, 9, 40)  # the MFE kernel scans special-hairpin keys in blocks of eight
_CANON = ("CG", "GC", "GU", "UG", "AU", "UA")
_MM = ("mismatchI", "mismatchH", "mismatchM", "mismatch1nI", "mismatch23I", "mismatchExt")
_SPECIALS = (("tetra_seq", "tetra_E", "n_tetra", 6), ("tri_seq", "tri_E", "n_tri", 5), ("hexa_seq", "hexa_E", "n_hexa", 8))


def _special_seqs(rng, n, length, taken):
    """n distinct loop strings of `length` letters closed by a canonical pair, none of them in `taken`."""
    out = []
    while len(out) < n:
        cp = _CANON[rng.integers(0, 6)]
        s = cp[0] + "".join("ACGU"[k] for k in rng.integers(0, 4, length - 2)) + cp[1]
        if s not in taken:
            taken.add(s)
            out.append(s)
    return out


def random_params_full(seed, counts=None):
    """params.random_params(seed) with EVERY field the model reads randomised as well: hairpin[3..30], bulge[1..30],
    internal_loop[2..30], lxc, ninio / max_ninio, MLintern per pair type, MLbase and TerminalAU of either sign, MLclosing,
    the dangles, the six mismatch tables and the special hairpins — energies and sequences, each closed by a canonical pair,
    all 40 slots filled (a reader past n_* finds plausible keys there), n_tetra / n_tri / n_hexa drawn from SPECIAL_COUNTS
    unless `counts` = (n_tetra, n_tri, n_hexa) is given.  Keeps the symmetries of random_params; its stacks are halved.  Every finite entry, the
    hairpin initiation extrapolated to 256 nt included, stays within SF_FAST_MAXPARAM, so W <= 256 runs on the int16 kernel."""
    from scanfold_amd import params
    p = params.random_params(seed)
    r = p.rec
    rng = np.random.default_rng([seed, 0x7ab1e5])
    r["stack"] = r["stack"] // 2  # (random_params' stacks alone fold 256-mers below the int16 kernel's range)
    r["hairpin"][3:31] = rng.integers(150, 800, 28)
    r["bulge"][1:31] = rng.integers(0, 700, 30)
    r["internal_loop"][2:31] = rng.integers(0, 700, 29)
    r["lxc"] = float(rng.uniform(40.0, 160.0))
    r["ninio"] = int(rng.integers(0, 120))
    r["max_ninio"] = int(rng.integers(0, 500))
    ml = rng.integers(-250, 60, 8)
    if (ml[1:8] == ml[1]).all():
        ml[2] += 37
    r["MLintern"] = ml
    r["MLbase"] = int(rng.integers(-40, 50))
    r["TerminalAU"] = int(rng.integers(-80, 120))
    r["MLclosing"] = int(rng.integers(-300, 1000))
    r["dangle5"] = rng.integers(-100, 30, (8, 5))
    r["dangle3"] = rng.integers(-100, 30, (8, 5))
    for f in _MM:
        r[f] = rng.integers(-150, 60, (8, 5, 5))
    if counts is None:
        counts = [SPECIAL_COUNTS[k] for k in rng.integers(0, len(SPECIAL_COUNTS), 3)]
    taken = set()
    for (fseq, fe, fn, ln), n in zip(_SPECIALS, counts):
        r[fseq] = [s.encode() for s in _special_seqs(rng, params.MAX_SPECIAL, ln, taken)]
        r[fe] = rng.integers(-500, 500, params.MAX_SPECIAL)
        r[fn] = int(n)
    p.source = "random_params_full(%d)" % seed
    return p


def boundary_params(seed, top=SF_FAST_MAXPARAM):
    """random_params_full(seed) with one MLintern for every pair type (the int16 kernel's condition besides magnitude) and
    its largest entries at +SF_FAST_MAXPARAM: ninio and max_ninio, every third internal_loop size, every fourth mismatchI
    entry, the odd hairpin sizes 3..29.  top > SF_FAST_MAXPARAM puts that value on ONE entry, internal_loop[17]: the set then
    goes to the int32 kernel at every width."""
    p = random_params_full(seed)
    r = p.rec
    r["MLintern"] = r["MLintern"][1]
    M = SF_FAST_MAXPARAM
    r["ninio"] = M
    r["max_ninio"] = M
    r["internal_loop"][4:31:3] = M
    mi = r["mismatchI"].copy()
    mi.reshape(-1)[::4] = M
    r["mismatchI"] = mi
    r["hairpin"][3:30:2] = M
    r["internal_loop"][17] = top
    p.source = "boundary_params(%d, %d)" % (seed, top)
    return p


def max_finite_entry(rec, W=256):
    """Largest |entry| below INF that the int16 kernel's magnitude check sees (sf_fast_build_params), with the hairpin
    initiation extrapolated to W nucleotides."""
    fields = ("stack", "hairpin", "bulge", "internal_loop", "dangle5", "dangle3", "int11", "int21", "int22", "ninio",
              "max_ninio", "MLbase", "MLclosing", "MLintern", "TerminalAU", "tetra_E", "tri_E", "hexa_E") + _MM
    v = np.concatenate([np.abs(np.asarray(rec[f], dtype=np.int64)).reshape(-1) for f in fields])
    ext = int(rec["hairpin"][30]) + int(float(rec["lxc"]) * np.log(W / 30.0))
    return max(int(v[v < INF].max()), abs(ext))


def plant_specials(rng, arr, p, per_row=3):
    """A copy of `arr` (uint8 ASCII, (n, W)) with special-hairpin strings of `p` written over each row at random places:
    mostly entries in use (slot < n_*), some from the unused slots behind them (they must NOT count)."""
    used, unused = [], []
    for fseq, _, fn, _ in _SPECIALS:
        n = int(p.rec[fn])
        for k, s in enumerate(p.rec[fseq]):
            (used if k < n else unused).append(bytes(s))
    out = np.array(arr, dtype=np.uint8, copy=True)
    W = out.shape[1]
    for row in out:
        for _ in range(per_row):
            pool = used if used and (not unused or rng.random() < 0.8) else unused
            s = pool[int(rng.integers(0, len(pool)))]
            at = int(rng.integers(0, W - len(s) + 1))
            row[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


def random_enthalpies(rec, seed):
    """synthetic_enthalpies with the scalar fields random too (MLintern per pair type): for ParamSet.at_temperature."""
    rng = np.random.default_rng([seed, 0xe47])
    dH = synthetic_enthalpies(rec, seed)
    for f in ("ninio", "MLbase", "MLclosing", "TerminalAU", "DuplexInit"):
        dH[f] = 3 * int(rec[f]) - int(rng.integers(0, 40)) * 10
    dH["MLintern"] = 3 * rec["MLintern"].astype(np.int64) - rng.integers(0, 40, 8) * 10
    return dH


def synthetic_enthalpies(rec, seed=0):
    """An enthalpy record shaped like Turner's: dH ~ 3 x dG - noise (keeps INF where dG is INF)."""
    rng = np.random.default_rng(seed)
    dH = np.zeros((), dtype=rec.dtype)
    for f in ("stack", "hairpin", "bulge", "internal_loop", "mismatchI", "mismatchH", "mismatchM", "mismatch1nI",
              "mismatch23I", "mismatchExt", "dangle5", "dangle3", "int11", "int21", "int22", "tetra_E", "tri_E", "hexa_E"):
        g = rec[f].astype(np.int64)
        v = 3 * g - rng.integers(0, 40, size=g.shape) * 10
        dH[f] = np.where(np.abs(g) >= INF, g, v)
    dH["ninio"] = 320
    dH["MLbase"] = 0
    dH["MLclosing"] = 3000
    dH["MLintern"][:] = -220
    dH["TerminalAU"] = 370
    dH["DuplexInit"] = 360
    return dH
